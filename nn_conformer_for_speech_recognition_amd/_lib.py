"""ctypes binding of libcfm.so — the C ABI declared in include/cfm.h.

The library is the product: if it is missing, or no GPU is visible, every op raises.  There
is no CPU / PyTorch fallback anywhere on the hot path.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch  # noqa: F401  (load torch's libamdhip64 first: libcfm resolves to the same runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFM_LIB") or os.path.join(_HERE, "libcfm.so")   # CFM_LIB: A/B builds only
CSRC = os.path.join(_HERE, "csrc")

F32, BF16, FP8 = 0, 1, 2
ACT_NONE, ACT_SILU = 0, 1

c_void_p, c_int, c_long, c_float, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t
c_u64 = ctypes.c_uint64


class NGramLMDesc(ctypes.Structure):
    """cfm_ngram_lm (include/cfm.h)."""
    _fields_ = [("unigrams", c_void_p), ("table", c_void_p), ("seed", c_u64), ("mask", ctypes.c_uint32),
                ("probe", c_int), ("order", c_int), ("V", c_int)]


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int), ("N", c_int), ("K", c_int), ("batch", c_int),
        ("dtype_ab", c_int),
        ("A", c_void_p), ("lda", c_long), ("stride_a", c_long), ("a_kmajor", c_int),
        ("B", c_void_p), ("ldb", c_long), ("stride_b", c_long), ("b_kmajor", c_int),
        ("C", c_void_p), ("ldc", c_long), ("stride_c", c_long), ("dtype_c", c_int),
        ("alpha", c_float),
        ("bias", c_void_p),
        ("act", c_int),
        ("act_grad", c_int),
        ("pre", c_void_p), ("dtype_pre", c_int),
        ("drop_p", c_float), ("drop_seed", c_u64), ("drop_offset", c_u64),
        ("out_scale", c_float),
        ("residual", c_void_p), ("ldr", c_long), ("dtype_r", c_int),
        ("split_k", c_int),
        ("workspace", c_void_p),
        ("probe", c_void_p),
        ("a_colsum", c_void_p),
        ("rowdot_with", c_void_p), ("rowdot_out", c_void_p), ("rowdot_T", c_int),
        ("alpha_a_dev", c_void_p), ("alpha_b_dev", c_void_p),
        ("allow_overlap", c_int),
        ("mx_a", c_void_p), ("mx_b", c_void_p),
        ("mx_out", c_void_p), ("mx_out_scales", c_void_p),
    ]


class GemmChoice(ctypes.Structure):
    """cfm_gemm_choice (include/cfm.h): what cfm_gemm_plan says a cfm_gemm call would launch."""
    _fields_ = [("variant", c_int), ("epilogue", c_int), ("grid_x", ctypes.c_uint), ("grid_y", ctypes.c_uint),
                ("grid_z", ctypes.c_uint), ("block", ctypes.c_uint)]


# Mirrors of the enums of include/cfm.h (tests/test_gemm_plan_cpu.py holds them equal to the header).
# cfm_gemm_mode (cfm_gemm_set_mode) and cfm_gemm_sel (its selector field, GEMM_SEL_* << GEMM_MODE_SEL_SHIFT)
GEMM_MODE_STAGED256 = 1 << 0
GEMM_MODE_PIPE = 1 << 1
GEMM_MODE_DEFAULT = 3
GEMM_MODE_SKIP_STORES = 1 << 3
GEMM_MODE_SEL_SHIFT = 4
GEMM_MODE_SEL_MASK = 7 << 4
GEMM_MODE_GENERIC_DROPOUT = 1 << 10
GEMM_MODE_NO_192S8_RULE = 1 << 12
GEMM_MODE_SKIP_MAINLOOP = 1 << 13
GEMM_MODE_GENERIC_EPILOGUE = 1 << 14
GEMM_MODE_KEEP_SHARED_DMA = 1 << 19
GEMM_MODE_KEEP_PIPE192 = 1 << 21
GEMM_MODE_KEEP_128WIDE = 1 << 22
GEMM_MODE_KEEP_WS192 = 1 << 23
GEMM_SEL_AUTO, GEMM_SEL_PIPE256, GEMM_SEL_PIPE256S, GEMM_SEL_192, GEMM_SEL_PIPE192S8 = 0, 1, 2, 5, 7
# cfm_gemm_variant
(GEMM_V_NONE, GEMM_V_STAGED_BF16_256, GEMM_V_STAGED_BF16_128, GEMM_V_STAGED_F32_128, GEMM_V_STAGED_F32_64,
 GEMM_V_PIPE64X160, GEMM_V_WS192, GEMM_V_WS96, GEMM_V_PIPE192, GEMM_V_PIPE192S8, GEMM_V_PIPE256, GEMM_V_PIPE256S,
 GEMM_V_FP8_192, GEMM_V_FP8_256S, GEMM_V_MX192, GEMM_V_MX256S) = range(16)
# cfm_gemm_epilogue
(GEMM_EPI_GENERIC, GEMM_EPI_BF16, GEMM_EPI_BF16_BIAS, GEMM_EPI_BF16_SILU, GEMM_EPI_BF16_ACTG, GEMM_EPI_BF16_RD,
 GEMM_EPI_F32, GEMM_EPI_F32_RES, GEMM_EPI_BF16_SILU_MX, GEMM_EPI_BF16_RES, GEMM_EPI_F32R_BF16,
 GEMM_EPI_BF16_DELTA) = range(12)
# cfm_convmod_op / cfm_convmod_family / cfm_convmod_apply (cfm_convmod_plan)
CONVMOD_OP_FWD, CONVMOD_OP_BWD, CONVMOD_OP_BWD_BN, CONVMOD_OP_BWD_GN = range(4)
CONVMOD_FAM_UNSUPPORTED, CONVMOD_FAM_VEC, CONVMOD_FAM_SCALAR_KT, CONVMOD_FAM_SCALAR_KRT = range(4)
CONVMOD_APPLY_NONE, CONVMOD_APPLY_SCALAR, CONVMOD_APPLY_VEC8 = range(3)
# cfm_attn_mode (cfm_attn_set_mode)
ATTN_MODE_TILED = 1 << 0
ATTN_MODE_STAGING_ONLY = 1 << 1
ATTN_MODE_SKIP_STORES = 1 << 2
ATTN_MODE_REL_SIMT = 1 << 4
ATTN_MODE_REL_ZERO_FILL = 1 << 6
ATTN_MODE_REL_DPOS_R4 = 1 << 7
ATTN_MODE_REL_DQ_RECOMPUTE = 1 << 9
ATTN_MODE_DQ_RECOMPUTE = 1 << 10
ATTN_MODE_DKDV_TWO_PASS = 1 << 11
# cfm_attn_path / cfm_attn_dpos / cfm_attn_ws (cfm_attn_plan)
ATTN_PATH_SIMT, ATTN_PATH_HEAD, ATTN_PATH_TILED, ATTN_PATH_REL = range(4)
ATTN_DPOS_NONE, ATTN_DPOS_XCD, ATTN_DPOS_R4_VEC, ATTN_DPOS_R4 = range(4)
ATTN_WS_D, ATTN_WS_PART, ATTN_WS_DS, ATTN_WS_DPOS = range(4)


class AttnQuery(ctypes.Structure):
    """cfm_attn_query (include/cfm.h): one attention call as cfm_attn_plan reads it."""
    _fields_ = [(n, c_int) for n in ("B", "T", "H", "dk", "dtype", "rel", "qkv_mod16", "dout_mod16", "pos_mod16",
                                     "mode", "cus")] + [("ws_bytes", ctypes.c_int64)]


class AttnChoice(ctypes.Structure):
    """cfm_attn_choice (include/cfm.h)."""
    _fields_ = [(n, c_int) for n in ("path", "vec", "vec4", "pvec", "rel_vec", "dbg", "qs", "waves", "dq_stored",
                                     "dpos")] + [(n, c_size_t) for n in ("lds_head", "lds_dkdv", "lds_dqs")] + [
        ("ws_off", c_size_t * 4), ("ws_size", c_size_t * 4), ("ws_total", c_size_t)]


# cfm_ln_op / cfm_ln_family (cfm_layernorm_plan)
LN_FWD, LN_FWD_RES, LN_BWD, LN_FWD_PAIR, LN_BWD_PAIR = range(5)
LN_GENERIC, LN_WAVE, LN_GROUP = range(3)


class LnQuery(ctypes.Structure):
    """cfm_ln_query (include/cfm.h): one LayerNorm call as cfm_layernorm_plan reads it."""
    _fields_ = [("op", c_int), ("D", c_int), ("M", ctypes.c_int64)] + [(n, c_int) for n in (
        "dt_x", "dt_y", "dt_dy", "dt_dx", "dt_dres", "dt_delta",
        "x_mod16", "y_mod16", "z_mod16", "gamma_mod16", "beta_mod16", "gamma2_mod16", "beta2_mod16",
        "delta_mod16", "xout_mod16", "y8_mod16", "dy_mod16", "dres_mod16", "dx_mod16", "g2_mod16",
        "want_mx", "want_g2")]


class LnChoice(ctypes.Structure):
    """cfm_ln_choice (include/cfm.h)."""
    _fields_ = [(n, c_int) for n in ("family", "width", "g2_fused", "blocks")] + [("ws_bytes", c_size_t)]


class ConvmodQuery(ctypes.Structure):
    """cfm_convmod_query (include/cfm.h): one conv-module launch as cfm_convmod_plan reads it."""
    _fields_ = [("op", c_int), ("norm", c_int), ("dtype_a", c_int), ("dtype_da", c_int), ("dtype_dz", c_int),
                ("dtype_z", c_int), ("M", c_long), ("C", c_int), ("K", c_int), ("y", c_void_p), ("z", c_void_p),
                ("force_scalar", c_int)]


class ConvmodChoice(ctypes.Structure):
    """cfm_convmod_choice (include/cfm.h)."""
    _fields_ = [("family", c_int), ("dz16", c_int), ("apply", c_int)]


class FfoldGeo(ctypes.Structure):
    """cfm_ffold_geo (include/cfm.h): the folded front-end geometry; cfm_ffold_geometry fills the derived fields."""
    _fields_ = [(n, c_int) for n in ("B", "F", "T", "C1", "C2", "D", "k1", "s1", "k2", "s2", "dtype", "hilo",
                                     "F2", "T2", "Ke", "Se", "Fp", "Cx", "Kp", "lda", "T2p", "Tslot")] + [
        ("xt_elems", c_long), ("ws_floats", c_long)]


class AdafactorParam(ctypes.Structure):
    """cfm_adafactor_param (include/cfm.h): one parameter as cfm_adafactor_plan / _fill_table read it."""
    _fields_ = [(n, c_void_p) for n in ("p", "g", "m", "row", "col")] + [("numel", c_long)] + [
        (n, c_int) for n in ("nb", "R", "C", "factored")]


class AdafactorTotals(ctypes.Structure):
    """cfm_adafactor_totals (include/cfm.h): the plan's sums over a group, or those in front of one parameter."""
    _fields_ = [(n, c_long) for n in ("row_tasks", "cols", "blocks", "rowmean_tasks", "colpart_tasks",
                                      "rowmean_floats", "part_floats")]


class AdafactorBuffers(ctypes.Structure):
    """cfm_adafactor_buffers (include/cfm.h)."""
    _fields_ = [(n, c_void_p) for n in ("rowmean", "part", "partial", "partial_p", "rms_out")]


class AdafactorHyper(ctypes.Structure):
    """cfm_adafactor_hyper (include/cfm.h): the scalars and variant flags of one cfm_adafactor_step."""
    _fields_ = [("decay_rate", ctypes.c_double)] + [(n, c_float) for n in (
        "lr", "beta1", "beta2t", "eps1", "eps2", "clip", "weight_decay")] + [
        ("flags", c_int), ("step_dev", c_void_p), ("scalars_dev", c_void_p)]


# cfm_adafactor_flags
ADA_SCALE_PARAMETER, ADA_RELATIVE_STEP, ADA_WARMUP_INIT, ADA_DEVICE_STEP = 1, 2, 4, 8


# name -> (restype, argtypes)
_SIGS = {
    "cfm_version": (c_int, []),
    "cfm_get_last_error": (ctypes.c_char_p, []),
    "cfm_rng_bind": (c_int, [c_void_p]),
    "cfm_probe_slot": (c_int, [c_void_p, c_int, c_void_p]),
    "cfm_wallclock_khz": (c_int, []),
    "cfm_cast": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_void_p]),
    "cfm_cast_batch": (c_int, [c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "cfm_cast_transpose_batch": (c_int, [c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "cfm_specaug_apply": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_void_p]),
    "cfm_logmel_ws_bytes": (c_size_t, [c_int, c_int]),
    "cfm_logmel_fwd": (c_int, [c_void_p, c_long, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "cfm_gemm": (c_int, [ctypes.POINTER(GemmDesc), c_void_p]),
    "cfm_gemm_set_mode": (c_int, [c_int]),
    "cfm_gemm_plan": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "cfm_quant_fp8": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_quant_fp8_ws_bytes": (c_size_t, []),
    "cfm_quant_fp8_batch_blocks": (c_long, [c_long]),
    "cfm_quant_fp8_batch": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p]),
    "cfm_dequant_fp8": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "cfm_layernorm_fwd_mx": (c_int, [c_void_p] * 8 + [c_long, c_int, c_float, c_void_p]),
    "cfm_layernorm_fwd_mx_ex": (c_int, [c_void_p, c_int] + [c_void_p] * 7 + [c_long, c_int, c_float, c_void_p]),
    "cfm_layernorm_fwd_res": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_float, c_void_p]),
    "cfm_quant_mx": (c_int, [c_void_p, c_int, c_long, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    "cfm_quant_mx_batch_blocks": (c_long, [c_long, c_int]),
    "cfm_quant_mx_batch": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p]),
    "cfm_dequant_mx": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "cfm_wgrad_group_task_bytes": (c_size_t, []),
    "cfm_wgrad_group_tiles": (c_long, [c_int, c_int]),
    "cfm_wgrad_group_fill": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_long]),
    "cfm_wgrad_group": (c_int, [c_void_p, c_int, c_long, c_void_p]),
    "cfm_wgrad_group_probed": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p]),
    "cfm_wgrad_group_plan": (c_long, [c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p]),
    "cfm_wgrad_group_ws_floats": (c_long, [c_int, c_int, c_int]),
    "cfm_wgrad_group_red_blocks": (c_long, [c_int, c_int, c_int]),
    "cfm_wgrad_group_fill_split": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                           c_int, c_int, c_void_p, c_long]),
    "cfm_wgrad_group_sched": (c_int, [c_void_p, c_int, c_void_p, c_long, c_long, c_void_p, c_void_p]),
    "cfm_colreduce_group_task_bytes": (c_size_t, []),
    "cfm_colreduce_group_blocks": (c_long, [c_long]),
    "cfm_colreduce_group_fill": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_long, c_void_p, c_void_p, c_int,
                                         c_int, c_int, c_long]),
    "cfm_colreduce_group": (c_int, [c_void_p, c_int, c_long, c_void_p]),
    "cfm_attn_set_mode": (c_int, [c_int]),
    "cfm_attn_plan": (c_int, [c_void_p, c_void_p]),
    "cfm_colreduce": (c_int, [c_void_p, c_int, c_long, c_long, c_void_p, c_int, c_void_p]),
    "cfm_colsum": (c_int, [c_void_p, c_int, c_long, c_int, c_long, c_void_p, c_int, c_void_p, c_void_p]),
    "cfm_layernorm_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_long, c_int, c_float, c_void_p]),
    "cfm_layernorm_ws_bytes": (c_size_t, [c_long, c_int]),
    "cfm_layernorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "cfm_layernorm_bwd_drop": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p,
                                       c_float, c_float, c_u64, c_void_p]),
    "cfm_layernorm_plan": (c_int, [ctypes.POINTER(LnQuery), ctypes.POINTER(LnChoice)]),
    "cfm_layernorm_pair_ok": (c_int, [c_int, c_int]),
    "cfm_layernorm_fwd_pair_ws_bytes": (c_size_t, [c_long, c_int]),
    "cfm_layernorm_fwd_pair": (c_int, [c_void_p] * 7 + [c_int] + [c_void_p] * 4 + [c_long, c_int, c_float, c_void_p]),
    "cfm_layernorm_bwd_pair_ws_bytes": (c_size_t, [c_long, c_int]),
    "cfm_layernorm_bwd_pair": (c_int, [c_void_p, c_int] + [c_void_p] * 13 + [c_long, c_int, c_void_p, c_float, c_float,
                                                                          c_u64, c_void_p]),
    "cfm_scale_dropout": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_float, c_float, c_u64, c_u64,
                                  c_void_p]),
    "cfm_convmod_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "cfm_convmod_nparts": (c_long, [c_int, c_int]),
    "cfm_convmod_plan": (c_int, [c_void_p, c_void_p]),
    "cfm_glu_dwconv_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "cfm_bn_silu_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int,
                                c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cfm_bn_silu_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cfm_bn_silu_fwd_sums": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cfm_bn_silu_fwd_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p,
                                      c_long, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "cfm_bn_silu_bwd_sums": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_bn_silu_bwd_apply": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_long, c_void_p, c_long, c_int, c_void_p]),
    "cfm_adafactor_table_bytes": (c_size_t, [c_int]),
    "cfm_adafactor_plan": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),    # (params, n, before or NULL, totals)
    "cfm_adafactor_fill_table": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "cfm_adafactor_step": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_silu_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_long, c_void_p]),
    "cfm_bn_ws_bytes": (c_size_t, [c_int]),
    "cfm_bn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_void_p,
                           c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p]),
    "cfm_bn_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                           c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cfm_glu_dwconv_bwd_bn": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_float, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                      c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cfm_gn_silu_fwd": (c_int, [c_void_p] * 3 + [c_float] + [c_void_p] * 3 + [c_int] * 4 + [c_void_p] * 2),
    "cfm_gn_silu_bwd_sums": (c_int, [c_void_p, c_int] + [c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 5),
    "cfm_gn_silu_bwd": (c_int, [c_void_p, c_int] + [c_void_p] * 9 + [c_int] * 3 + [c_void_p] * 2),
    "cfm_glu_dwconv_bwd_gn": (c_int, [c_void_p, c_int] + [c_void_p] * 7 + [c_int, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cfm_glu_dwconv_bwd_wgrad": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "cfm_glu_dwconv_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cfm_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                             c_int, c_int, c_int, c_float, c_u64, c_void_p]),
    "cfm_attn_bwd_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "cfm_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                             c_u64, c_void_p, c_size_t, c_void_p]),
    "cfm_attn_bwd_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                c_float, c_u64, c_int, c_void_p, c_size_t, c_void_p]),
    "cfm_conv1_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "cfm_conv2_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_void_p]),
    "cfm_conv2_bwd_data": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p]),
    "cfm_conv2_bwd_data_ws_bytes": (c_size_t, [c_int, c_int]),
    "cfm_conv2_bwd_data_ws": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_void_p]),
    "cfm_conv2_bwd_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    "cfm_conv2_bwd_weight_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "cfm_conv2_bwd_weight_ws": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p]),
    "cfm_ctc_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "cfm_ctc_mean": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_bind_abort_counter": (c_int, [c_void_p]),
    "cfm_ctc_set_debug": (c_int, [c_int]),
    "cfm_ctc_loss_fwd": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_loss_bwd": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_long,
                                 c_long, c_void_p]),
    "cfm_ctc_greedy_decode": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_beam_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "cfm_ctc_beam_decode": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_beam_lm_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "cfm_ctc_beam_decode_lm": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_float, c_float, c_int, ctypes.POINTER(NGramLMDesc), c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_align_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "cfm_ctc_forced_align": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                     c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    "cfm_ctc_nbest_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),   # (B, T, N, max_labels)
    # (logits, sb, st, in_len, B, T, V, hyp, ldh, hyp_len, N, max_labels, blank, risk, ll, post, loss, ws, stream)
    "cfm_ctc_nbest_fwd": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # (the same through blank, ws, grad_loss, grad_stride, grad_logits, gsb, gst, stream)
    "cfm_ctc_nbest_bwd": (c_int, [c_void_p, c_long, c_long, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_long, c_long,
                                  c_void_p]),
    "cfm_rnnt_ws_bytes": (c_size_t, [c_int, c_int, c_int]),   # (B, T, U1)
    # (logits, targets, ldt, in_len, tgt_len, B, T, U1, V, blank, ll, ws, stream)
    "cfm_rnnt_loss_fwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p]),
    # (the same through blank, ws, grad_loss, dlogits, stream)
    "cfm_rnnt_loss_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    # (ep, gtab, w_hh, w_pp, b_pp, w_out, b_out, lengths, B, T, V, H, J, blank, max_symbols, W, tokens, frames, counts,
    #  scores, stream)
    "cfm_rnnt_greedy": (c_int, [c_void_p] * 8 + [c_int] * 8 + [c_void_p] * 5),
    "cfm_edit_distance_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),   # (P, Rmax, Hmax, want_ops)
    # (ref, ldr, ref_len, n_ref, hyp, ldh, hyp_len, P, group, Rmax, Hmax, dist, counts, pair_ref, pair_hyp, ldp,
    #  n_pairs, ws, stream)
    "cfm_edit_distance": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "cfm_lstm_ws_bytes": (c_size_t, [c_int, c_int]),   # (H, ndir)
    "cfm_lstm_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                             c_void_p]),
    "cfm_lstm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                             c_void_p]),
    "cfm_lstm_batched_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),   # (B, T, H, ndir)
    # (gx, whh, lengths, y, gates, c, hprev, B, T, stride_b, stride_t, H, ndir, ws, stream)
    "cfm_lstm_batched_fwd": (c_int, [c_void_p] * 7 + [c_int, c_int, c_long, c_long, c_int, c_int, c_void_p,
                                                      c_void_p]),
    # (dy, whh_t, gates, c, lengths, dg, B, T, stride_b, stride_t, H, ndir, ws, stream)
    "cfm_lstm_batched_bwd": (c_int, [c_void_p] * 6 + [c_int, c_int, c_long, c_long, c_int, c_int, c_void_p,
                                                      c_void_p]),
    "cfm_ffold_geometry": (c_int, [c_void_p]),
    "cfm_ffold_pack": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "cfm_ffold_compose": (c_int, [c_void_p] * 11),
    "cfm_ffold_bwd_weights": (c_int, [c_void_p] * 14),
    "cfm_conv1_bwd_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "cfm_conv1_bwd_weight": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p]),
}

EXPORTED = sorted(k for k in _SIGS)

_lib = None
MISSING = []


class CfmError(RuntimeError):
    pass


def build(verbose=False):
    """Compile libcfm.so in-tree with hipcc for gfx950 (make -C csrc)."""
    jobs = str(min(16, os.cpu_count() or 4))
    r = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise CfmError("libcfm build failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


def load():
    """Load libcfm.so (no GPU work); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CfmError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc, gfx950). There is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name, None)
        if fn is None:
            MISSING.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# True while a device dropout step counter is bound (cfm_rng_bind with a non-NULL pointer): the compiled
# encoder route (Conformer._forward_tokens_ops) needs it for fresh masks per step
RNG_BOUND = False


def call(name, *args):
    global RNG_BOUND
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.cfm_get_last_error().decode(errors="replace")
        raise CfmError(f"{name} failed ({rc}): {msg}")
    if name == "cfm_rng_bind":
        RNG_BOUND = bool(args and args[0])
    return rc


def size_call(name, *args):
    return int(getattr(load(), name)(*args))


def ptr(t):
    """Device pointer of a tensor (or None -> NULL). Tensors must live on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise CfmError("cfm ops need GPU tensors (the HIP path has no CPU fallback)")
    return t.data_ptr()


def dt(t):
    if t is None:
        return F32
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype in (torch.uint8, torch.float8_e4m3fn):
        return FP8
    raise CfmError(f"unsupported dtype {t.dtype}")


def stream():
    return torch.cuda.current_stream().cuda_stream
