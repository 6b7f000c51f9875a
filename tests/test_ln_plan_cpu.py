"""cfm_layernorm_plan: which LayerNorm kernel a call runs, its grid, its workspace and where g2 comes from, pinned
without a GPU.  Every cfm_layernorm_* entry point, the *_ws_bytes functions and cfm_layernorm_pair_ok call the same
routine (csrc/ln_plan.h), so these rows are the launches.  The expectations are typed in from the rule as
include/cfm.h and DESIGN.md state it; blocks and ws_bytes are worked out by hand in the comments."""
import ctypes

import pytest

from nn_conformer_for_speech_recognition_amd import _lib as L

F32, BF16, FP8 = L.F32, L.BF16, L.FP8
FWD, RES, BWD, FPAIR, BPAIR = L.LN_FWD, L.LN_FWD_RES, L.LN_BWD, L.LN_FWD_PAIR, L.LN_BWD_PAIR
SHAPE, DTYPE, ALIGN = -2, -3, -4


def _query(op, M, D, x=F32, y=F32, dy=F32, dx=F32, dres=F32, delta=BF16, mx=0, g2=0, **mod16):
    q = L.LnQuery(op=op, D=D, M=M, dt_x=x, dt_y=y, dt_dy=dy, dt_dx=dx, dt_dres=dres, dt_delta=delta, want_mx=mx,
                  want_g2=g2)
    for name, v in mod16.items():          # x=..., gamma=... would clash with the dtypes: the fields' own names
        assert name.endswith("_mod16")
        setattr(q, name, v)
    return q


def _plan(q):
    c = L.LnChoice()
    rc = L.load().cfm_layernorm_plan(ctypes.byref(q), ctypes.byref(c))
    return rc, c


def wave(V, blocks, ws=0, g2=0):
    return (L.LN_WAVE, V, g2, blocks, ws)


def group(G, blocks, ws=0, g2=0):
    return (L.LN_GROUP, G, g2, blocks, ws)


def generic(blocks, ws=0):
    return (L.LN_GENERIC, 0, 0, blocks, ws)


# Forward blocks: ceil(M / rows), rows per workgroup = WAVE 8, GROUP 16 -> 32, 32 -> 16, 64 -> 8, GENERIC 4.
# Backward blocks nb = ceil(M / 16) clamped to [1, 1024]; ws = (nb + 1) * 8 D bytes, the pair's nb * 16 D.
#   M 777: nb 49; M 1000: nb 63; M 555: nb 35; M 37: nb 3; M 5: nb 1; M 1001: fwd 126
TABLE = [
    # ---- tests/test_gpu_kernels.py::test_layernorm: M 777, fp32 x, y / dy in both dtypes
    ("fwd-512", (FWD, 777, 512), {}, wave(8, 98)),
    ("fwd-512-bf16", (FWD, 777, 512), dict(y=BF16), wave(8, 98)),
    ("fwd-256", (FWD, 777, 256), {}, wave(4, 98)),
    ("fwd-128", (FWD, 777, 128), {}, wave(2, 98)),
    ("fwd-1024", (FWD, 777, 1024), dict(y=BF16), wave(16, 98)),
    ("fwd-144", (FWD, 777, 144), dict(y=BF16), group(32, 49)),              # 18 lanes of 8 -> G 32, 16 rows a block
    ("fwd-64", (FWD, 777, 64), {}, group(16, 25)),                          # G 16: 32 rows a block
    ("fwd-200", (FWD, 777, 200), {}, group(32, 49)),
    ("fwd-384", (FWD, 777, 384), {}, group(64, 98)),                        # 48 lanes -> G 64: 8 rows a block
    ("fwd-100", (FWD, 777, 100), {}, generic(195)),                         # no 16-byte vectors: 4 rows a block
    ("bwd-512", (BWD, 777, 512), {}, wave(8, 49, 204800)),                  # 50 * 8 * 512
    ("bwd-512-bf16", (BWD, 777, 512), dict(dy=BF16), wave(8, 49, 204800)),
    ("bwd-256", (BWD, 777, 256), {}, wave(4, 49, 102400)),
    ("bwd-128", (BWD, 777, 128), dict(dy=BF16), wave(2, 49, 51200)),
    ("bwd-1024", (BWD, 777, 1024), {}, wave(16, 49, 409600)),
    ("bwd-144", (BWD, 777, 144), dict(dy=BF16), group(32, 49, 57600)),
    ("bwd-64", (BWD, 777, 64), {}, group(16, 49, 25600)),
    ("bwd-200", (BWD, 777, 200), {}, group(32, 49, 80000)),
    ("bwd-384", (BWD, 777, 384), {}, group(64, 49, 153600)),
    ("bwd-100", (BWD, 777, 100), {}, generic(49, 40000)),
    # ---- test_layernorm's small M (a partial wave / slot) and its misaligned-x case
    ("fwd-144-M1", (FWD, 1, 144), {}, group(32, 1)),
    ("fwd-512-M9", (FWD, 9, 512), {}, wave(8, 2)),
    ("bwd-144-M9", (BWD, 9, 144), {}, group(32, 1, 2304)),                  # 2 * 8 * 144
    ("bwd-512-M1", (BWD, 1, 512), {}, wave(8, 1, 8192)),
    ("fwd-512-M37-x4", (FWD, 37, 512), dict(x_mod16=4), generic(10)),
    ("bwd-512-M37-x4", (BWD, 37, 512), dict(x_mod16=4), generic(3, 16384)),
    # ---- test_layernorm_bwd_fused_dropout_output: M 1000, bf16 dy, g2
    ("g2-512", (BWD, 1000, 512), dict(dy=BF16, g2=1), wave(8, 63, 262144, g2=1)),
    ("g2-144", (BWD, 1000, 144), dict(dy=BF16, g2=1), group(32, 63, 73728, g2=1)),
    ("g2-200", (BWD, 1000, 200), dict(dy=BF16, g2=1), group(32, 63, 102400, g2=1)),
    ("g2-100", (BWD, 1000, 100), dict(dy=BF16, g2=1), generic(63, 51200)),  # the separate pass
    # ---- tests/test_gpu_dropout_masks.py: M 37
    ("mask-fwd-144", (FWD, 37, 144), dict(y=BF16), group(32, 3)),
    ("mask-fwd-512", (FWD, 37, 512), dict(y=BF16), wave(8, 5)),
    ("mask-fwd-100", (FWD, 37, 100), dict(y=BF16), generic(10)),
    ("mask-bwd-144", (BWD, 37, 144), dict(dy=BF16, g2=1), group(32, 3, 4608, g2=1)),
    ("mask-bwd-512", (BWD, 37, 512), dict(dy=BF16, g2=1), wave(8, 3, 16384, g2=1)),
    ("mask-bwd-100", (BWD, 37, 100), dict(dy=BF16, g2=1), generic(3, 3200)),
    ("mask-fpair-144", (FPAIR, 37, 144), dict(y=BF16), group(32, 3)),
    ("mask-fpair-512", (FPAIR, 37, 512), dict(y=BF16), wave(8, 5)),
    ("mask-bpair-144", (BPAIR, 37, 144), dict(dy=BF16, g2=1), group(32, 3, 6912, g2=1)),
    ("mask-bpair-512", (BPAIR, 37, 512), dict(dy=BF16, g2=1), wave(8, 3, 24576, g2=1)),
    # ---- test_layernorm_bf16_residual_input: M 555, bf16 x
    ("bf16x-fwd-512", (FWD, 555, 512), dict(x=BF16, y=BF16), wave(8, 70)),
    ("bf16x-fwd-144", (FWD, 555, 144), dict(x=BF16, y=BF16), group(32, 35)),
    ("bf16x-fwd-256", (FWD, 555, 256), dict(x=BF16, y=BF16), wave(4, 70)),
    ("bf16x-fwd-100", (FWD, 555, 100), dict(x=BF16, y=BF16), generic(139)),
    ("bf16x-bwd-512", (BWD, 555, 512), dict(x=BF16), wave(8, 35, 147456)),
    ("bf16x-bwd-144", (BWD, 555, 144), dict(x=BF16), group(32, 35, 41472)),
    ("bf16x-mx-512", (FWD, 555, 512), dict(x=BF16, y=BF16, mx=1), wave(8, 70)),
    ("bf16x-mx-256", (FWD, 555, 256), dict(x=BF16, y=BF16, mx=1), wave(4, 70)),
    # ---- test_layernorm_fwd_residual_add: M 555, bf16 and fp32 delta, the MX copy
    ("res-512", (RES, 555, 512), dict(y=BF16), wave(8, 70)),
    ("res-256", (RES, 555, 256), {}, wave(4, 70)),
    ("res-144", (RES, 555, 144), dict(y=BF16), group(32, 35)),
    ("res-1024", (RES, 555, 1024), {}, wave(16, 70)),
    ("res-128", (RES, 555, 128), {}, wave(2, 70)),
    ("res-100", (RES, 555, 100), {}, generic(139)),
    ("res-512-f32delta", (RES, 555, 512), dict(delta=F32), generic(139)),
    ("res-144-f32delta", (RES, 555, 144), dict(delta=F32), generic(139)),
    ("res-mx-512", (RES, 555, 512), dict(y=BF16, mx=1), wave(8, 70)),
    ("res-mx-256", (RES, 555, 256), dict(y=BF16, mx=1), wave(4, 70)),
    ("res-mx-1024", (RES, 555, 1024), dict(y=BF16, mx=1), wave(16, 70)),
    # ---- tests/test_gpu_fp8.py: the MX forward at M 1001
    ("mx-256", (FWD, 1001, 256), dict(y=BF16, mx=1), wave(4, 126)),
    ("mx-512", (FWD, 1001, 512), dict(y=BF16, mx=1), wave(8, 126)),
    ("mx-1024", (FWD, 1001, 1024), dict(y=BF16, mx=1), wave(16, 126)),
    # ---- tests/test_gpu_ln_pair.py: D 512 / 256 / 144 at M 777 and 5, g2 always asked for
    ("fpair-512", (FPAIR, 777, 512), dict(y=BF16), wave(8, 98)),
    ("fpair-256", (FPAIR, 777, 256), {}, wave(4, 98)),
    ("fpair-144", (FPAIR, 777, 144), dict(y=BF16), group(32, 49)),
    ("fpair-512-M5", (FPAIR, 5, 512), {}, wave(8, 1)),
    ("fpair-256-M5", (FPAIR, 5, 256), {}, wave(4, 1)),
    ("fpair-144-M5", (FPAIR, 5, 144), {}, group(32, 1)),
    ("bpair-512", (BPAIR, 777, 512), dict(dy=BF16, g2=1), wave(8, 49, 401408, g2=1)),     # 49 * 16 * 512
    ("bpair-256", (BPAIR, 777, 256), dict(dy=BF16, g2=1), wave(4, 49, 200704, g2=0)),     # V 4: the separate pass
    ("bpair-144", (BPAIR, 777, 144), dict(g2=1), group(32, 49, 112896, g2=1)),
    ("bpair-512-M5", (BPAIR, 5, 512), dict(g2=1), wave(8, 1, 8192, g2=1)),
    ("bpair-256-M5", (BPAIR, 5, 256), dict(g2=1), wave(4, 1, 4096, g2=0)),
    ("bpair-144-M5", (BPAIR, 5, 144), dict(g2=1), group(32, 1, 2304, g2=1)),
    ("bpair-144-nog2", (BPAIR, 777, 144), dict(dy=BF16), group(32, 49, 112896)),
    # ---- the other lane-group widths have pairs too; D 128 / 1024 (V 2 / 16), 100 and 1032 have none
    ("fpair-64", (FPAIR, 777, 64), {}, group(16, 25)),
    ("fpair-200", (FPAIR, 777, 200), {}, group(32, 49)),
    ("bpair-384", (BPAIR, 777, 384), dict(g2=1), group(64, 49, 301056, g2=1)),
    ("fpair-128", (FPAIR, 777, 128), {}, SHAPE),
    ("bpair-128", (BPAIR, 777, 128), {}, SHAPE),
    ("fpair-1024", (FPAIR, 777, 1024), {}, SHAPE),
    ("fpair-100", (FPAIR, 8, 100), {}, SHAPE),
    ("bpair-1032", (BPAIR, 8, 1032), {}, SHAPE),
    ("fpair-0", (FPAIR, 8, 0), {}, SHAPE),
    # ---- D outside (0, 1024], M < 0
    ("fwd-1032", (FWD, 8, 1032), {}, SHAPE),
    ("bwd-1032", (BWD, 8, 1032), {}, SHAPE),
    ("res-0", (RES, 8, 0), {}, SHAPE),
    ("fwd-M-1", (FWD, -1, 512), {}, SHAPE),
    ("bpair-M-1", (BPAIR, -1, 512), {}, SHAPE),
    ("fwd-1000", (FWD, 37, 1000), {}, generic(10)),                         # D % 8 == 0 but > 512 and not 64 V
    # ---- one row per pointer whose misalignment demotes to GENERIC (M 37: fwd 10 blocks; bwd 3, ws 4 * 8 D)
    ("fwd-mis-x", (FWD, 37, 512), dict(x_mod16=8), generic(10)),
    ("fwd-mis-y", (FWD, 37, 512), dict(y_mod16=2), generic(10)),
    ("fwd-mis-gamma", (FWD, 37, 144), dict(gamma_mod16=4), generic(10)),
    ("fwd-mis-beta", (FWD, 37, 144), dict(beta_mod16=4), generic(10)),
    ("res-mis-delta", (RES, 37, 512), dict(delta_mod16=2), generic(10)),
    ("res-mis-xout", (RES, 37, 144), dict(xout_mod16=4), generic(10)),
    ("bwd-mis-dy", (BWD, 37, 512), dict(dy_mod16=8), generic(3, 16384)),
    ("bwd-mis-x", (BWD, 37, 144), dict(x_mod16=4), generic(3, 4608)),
    ("bwd-mis-dres", (BWD, 37, 512), dict(dres_mod16=4), generic(3, 16384)),
    ("bwd-mis-dx", (BWD, 37, 144), dict(dx_mod16=4), generic(3, 4608)),
    ("bwd-mis-gamma", (BWD, 37, 512), dict(gamma_mod16=4), generic(3, 16384)),
    ("fwd-mis-unused", (FWD, 37, 512), dict(dy_mod16=4, g2_mod16=4, z_mod16=4), wave(8, 5)),  # not the forward's pointers
    # ---- the pairs have no generic kernel: a misaligned pointer is refused
    ("fpair-mis-x", (FPAIR, 37, 512), dict(x_mod16=4), ALIGN),
    ("fpair-mis-z", (FPAIR, 37, 144), dict(z_mod16=8), ALIGN),
    ("fpair-mis-beta2", (FPAIR, 37, 144), dict(beta2_mod16=4), ALIGN),
    ("bpair-mis-dz", (BPAIR, 37, 512), dict(dy_mod16=8), ALIGN),
    ("bpair-mis-gamma2", (BPAIR, 37, 144), dict(gamma2_mod16=4), ALIGN),
    ("bpair-mis-g2", (BPAIR, 37, 144), dict(g2=1, g2_mod16=8), ALIGN),
    # ---- dtypes the fast kernels do not take: generic (x, dx, dres), fp32 delta above
    ("bwd-dx-bf16", (BWD, 37, 512), dict(dx=BF16), generic(3, 16384)),
    ("bwd-dres-bf16", (BWD, 37, 144), dict(dres=BF16), generic(3, 4608)),
    ("fwd-x-fp8", (FWD, 37, 512), dict(x=FP8), generic(10)),
    ("res-x-bf16", (RES, 37, 512), dict(x=BF16), generic(10)),              # (the entry point itself passes fp32)
    # ---- y / z / dy / dz (delta, the MX forward's x) outside {f32, bf16}: refused by every op
    ("fwd-y-fp8", (FWD, 37, 512), dict(y=FP8), DTYPE),
    ("fwd-y-fp8-100", (FWD, 37, 100), dict(y=FP8), DTYPE),
    ("res-y-7", (RES, 37, 512), dict(y=7), DTYPE),
    ("res-delta-fp8", (RES, 37, 512), dict(delta=FP8), DTYPE),
    ("bwd-dy-fp8", (BWD, 37, 512), dict(dy=FP8), DTYPE),
    ("bwd-dy-fp8-100", (BWD, 37, 100), dict(dy=-1), DTYPE),
    ("fpair-z-fp8", (FPAIR, 37, 512), dict(y=FP8), DTYPE),
    ("bpair-dz-fp8", (BPAIR, 37, 144), dict(dy=FP8), DTYPE),
    ("mx-x-fp8", (FWD, 37, 512), dict(x=FP8, y=BF16, mx=1), DTYPE),
    # ---- the MX copy: WAVE V >= 4 and a bf16 y only
    ("mx-128", (FWD, 37, 128), dict(y=BF16, mx=1), SHAPE),
    ("mx-144", (FWD, 37, 144), dict(y=BF16, mx=1), SHAPE),
    ("res-mx-128", (RES, 37, 128), dict(y=BF16, mx=1), SHAPE),
    ("res-mx-f32y", (RES, 37, 512), dict(y=F32, mx=1), SHAPE),
    ("mx-mis-x", (FWD, 37, 512), dict(y=BF16, mx=1, x_mod16=4), ALIGN),
    ("mx-mis-gamma", (FWD, 37, 256), dict(y=BF16, mx=1, gamma_mod16=8), ALIGN),
    ("mx-mis-y8", (FWD, 37, 512), dict(y=BF16, mx=1, y8_mod16=4), ALIGN),
    ("mx-y8-8", (FWD, 37, 512), dict(y=BF16, mx=1, y8_mod16=8), wave(8, 5)),                  # y8 moves 8-byte words
    ("res-mx-mis-delta", (RES, 37, 512), dict(y=BF16, mx=1, delta_mod16=2), ALIGN),
    ("res-mx-f32delta", (RES, 37, 512), dict(y=BF16, mx=1, delta=F32), ALIGN),
    ("res-mx-mis-y8", (RES, 37, 512), dict(y=BF16, mx=1, y8_mod16=4), SHAPE),                 # (fwd_res reports it so)
    # ---- g2: fused on V 8 and GROUP; V 16 and the pair's V 4 take the separate pass; a backward at D 128 / 256 with
    #      a g2 it can store runs that width's GROUP kernel (G 16 / 32), which has the epilogue
    ("g2-1024", (BWD, 37, 1024), dict(g2=1), wave(16, 3, 32768, g2=0)),
    ("g2-256", (BWD, 37, 256), dict(g2=1), group(32, 3, 8192, g2=1)),
    ("g2-128", (BWD, 37, 128), dict(g2=1), group(16, 3, 4096, g2=1)),
    ("g2-256-mis", (BWD, 37, 256), dict(g2=1, g2_mod16=2), wave(4, 3, 8192, g2=0)),
    ("g2-512-mis", (BWD, 37, 512), dict(g2=1, g2_mod16=8), wave(8, 3, 16384, g2=0)),
    ("g2-144-mis", (BWD, 37, 144), dict(g2=1, g2_mod16=8), group(32, 3, 4608, g2=0)),         # the kernel stays GROUP
    ("g2-512-mis-x", (BWD, 37, 512), dict(g2=1, x_mod16=4), generic(3, 16384)),
    ("nog2-g2mod", (BWD, 37, 256), dict(g2_mod16=0), wave(4, 3, 8192)),
    # ---- M = 0 (the forward launches nothing; the backward's one block writes zero partials) and the block cap
    ("fwd-M0", (FWD, 0, 512), {}, wave(8, 0)),
    ("fwd-M0-144", (FWD, 0, 144), {}, group(32, 0)),
    ("mx-M0-mis", (FWD, 0, 512), dict(y=BF16, mx=1, x_mod16=4), generic(0)),                  # nothing to launch
    ("bwd-M0", (BWD, 0, 512), {}, wave(8, 1, 8192)),
    ("bpair-M0", (BPAIR, 0, 144), {}, group(32, 1, 2304)),
    ("bwd-cap-1", (BWD, 16368, 512), {}, wave(8, 1023, 4194304)),                             # 1024 * 4096
    ("bwd-cap", (BWD, 16384, 512), {}, wave(8, 1024, 4198400)),                               # 1025 * 4096
    ("bwd-cap+1", (BWD, 16385, 144), {}, group(32, 1024, 1180800)),                           # 1025 * 1152
    ("bpair-cap", (BPAIR, 1 << 20, 512), {}, wave(8, 1024, 8388608)),                         # 1024 * 16 * 512
    ("fwd-big", (FWD, 1 << 20, 144), {}, group(32, 65536)),
]


@pytest.mark.parametrize("args,kw,want", [r[1:] for r in TABLE], ids=[r[0] for r in TABLE])
def test_choice(args, kw, want):
    lib = L.load()
    rc, c = _plan(_query(*args, **kw))
    if isinstance(want, int):
        assert rc == want
        assert lib.cfm_get_last_error()
        return
    assert rc == 0, lib.cfm_get_last_error()
    assert (c.family, c.width, c.g2_fused, c.blocks, c.ws_bytes) == want


def test_size_functions_answer_from_the_plan():
    """cfm_layernorm_ws_bytes / _bwd_pair_ws_bytes / _pair_ok against the table's rows and tests/test_ln_pair_cpu.py's
    numbers; where the entry point refuses the shape there is nothing to size."""
    lib = L.load()
    for _, (op, M, D), kw, want in TABLE:
        if isinstance(want, int) or kw.get("dy", F32) not in (F32, BF16):
            continue
        if op == BWD:
            assert lib.cfm_layernorm_ws_bytes(M, D) == want[4]
        elif op == BPAIR:
            assert lib.cfm_layernorm_bwd_pair_ws_bytes(M, D) == want[4]
            assert lib.cfm_layernorm_pair_ok(D, BF16) == 1
    assert lib.cfm_layernorm_bwd_pair_ws_bytes(777, 512) == 49 * 4 * 512 * 4
    assert lib.cfm_layernorm_bwd_pair_ws_bytes(5, 144) == 1 * 4 * 144 * 4
    assert lib.cfm_layernorm_ws_bytes(777, 512) == 49 * 2 * 512 * 4 + 2 * 512 * 4
    for D in (128, 1024, 100, 1032, 0):
        assert lib.cfm_layernorm_pair_ok(D, F32) == 0 and lib.cfm_layernorm_bwd_pair_ws_bytes(777, D) == 0
    assert lib.cfm_layernorm_ws_bytes(777, 1032) == 0 and lib.cfm_layernorm_ws_bytes(-1, 512) == 0
    assert lib.cfm_layernorm_pair_ok(512, FP8) == 0


def test_errors():
    lib = L.load()
    q, c = _query(FWD, 37, 512), L.LnChoice()
    assert lib.cfm_layernorm_plan(None, ctypes.byref(c)) == -1
    assert lib.cfm_layernorm_plan(ctypes.byref(q), None) == -1
    assert _plan(_query(5, 37, 512))[0] == -1 and _plan(_query(-1, 37, 512))[0] == -1       # unknown op
    # the dtype is reported before the shape, as cfm_layernorm_fwd_res always did
    assert _plan(_query(RES, 37, 0, delta=FP8))[0] == DTYPE
