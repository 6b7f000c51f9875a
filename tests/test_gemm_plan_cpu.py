"""cfm_gemm_plan: which kernel a cfm_gemm call runs, pinned without a GPU.  cfm_gemm and cfm_gemm_plan share one
preparation routine (csrc/gemm.hip gemm_prepare), so these rows are the launches.  Expected values are read off the
selection rules as they stood before they were gathered into one function."""
import ctypes
import os
import re

import pytest

from nn_conformer_for_speech_recognition_amd import _lib as L
from nn_conformer_for_speech_recognition_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, CUS = 11936, 256           # the encoder's token count (32 x 373); MI355X compute units
F32, BF16, FP8 = L.F32, L.BF16, L.FP8
D = L.GEMM_MODE_DEFAULT
PA, PB, PC, PX = 1 << 20, 2 << 20, 3 << 20, 4 << 20     # fake 4096-aligned pointers (never dereferenced)


def _desc(N, K, *, M=M, dt=BF16, a_kmajor=1, b_kmajor=1, dtype_c=BF16, lda=None, **kw):
    f = dict(M=M, N=N, K=K, batch=1, dtype_ab=dt, A=PA, lda=lda if lda is not None else (K if a_kmajor else M),
             a_kmajor=a_kmajor, B=PB, ldb=K if b_kmajor else N, b_kmajor=b_kmajor, C=PC, ldc=N, dtype_c=dtype_c,
             alpha=1.0, out_scale=1.0, ldr=N, split_k=1)
    f.update(kw)
    return ops._gemm_desc(**f)


def _plan(d, mode=D, cus=CUS):
    c = L.GemmChoice()
    rc = L.load().cfm_gemm_plan(ctypes.byref(d), mode, cus, ctypes.byref(c))
    assert rc == 0, L.load().cfm_get_last_error()
    return c


def _is(c, variant, grid=None, block=None, epi=None):
    assert c.variant == variant, c.variant
    if grid is not None:
        assert (c.grid_x, c.grid_y, c.grid_z) == tuple(grid) + (1,) * (3 - len(grid))
    if block is not None:
        assert c.block == block
    if epi is not None:
        assert c.epilogue == epi, c.epilogue


def _forced(sel):
    return L.GEMM_MODE_PIPE | sel << L.GEMM_MODE_SEL_SHIFT


DWIDE = dict(N=512, K=2048, dtype_c=F32, bias=PX, residual=PX + 4096, dtype_r=F32)
FFN_UP = dict(bias=PX, act=L.ACT_SILU, pre=PX + 4096, dtype_pre=BF16)


def test_encoder_shapes_default_mode():
    _is(_plan(_desc(**DWIDE)), L.GEMM_V_WS192, (4, 63), 768, L.GEMM_EPI_F32_RES)           # d-wide
    _is(_plan(_desc(256, 1024)), L.GEMM_V_WS96, (2, 125), 768, L.GEMM_EPI_BF16)              # Conformer-M width
    _is(_plan(_desc(144, 576)), L.GEMM_V_PIPE64X160, (1, 187), 320, L.GEMM_EPI_BF16)         # Conformer-S width
    _is(_plan(_desc(1536, 512, bias=PX)), L.GEMM_V_WS192, (12, 63), 768, L.GEMM_EPI_BF16_BIAS)   # QKV
    _is(_plan(_desc(576, 144)), L.GEMM_V_PIPE192S8, (5, 63), 512, L.GEMM_EPI_BF16)            # S FFN-up
    _is(_plan(_desc(2048, 512, **FFN_UP)), L.GEMM_V_PIPE256S, (16, 47), 512, L.GEMM_EPI_BF16_SILU)   # L FFN-up
    # the BK-64 256-row kernel exists with the generic epilogue only
    _is(_plan(_desc(2048, 2048, **FFN_UP)), L.GEMM_V_PIPE256, (16, 47), 512, L.GEMM_EPI_GENERIC)


def test_ab_bits_select_the_kept_variant():
    _is(_plan(_desc(**DWIDE), D | L.GEMM_MODE_KEEP_SHARED_DMA), L.GEMM_V_PIPE192, (4, 63), 512, L.GEMM_EPI_GENERIC)
    _is(_plan(_desc(256, 1024), D | L.GEMM_MODE_KEEP_WS192), L.GEMM_V_WS192, (2, 63), 768)
    _is(_plan(_desc(1536, 512), D | L.GEMM_MODE_KEEP_PIPE192), L.GEMM_V_PIPE192S8, (12, 63), 512)
    _is(_plan(_desc(1536, 512), D | L.GEMM_MODE_NO_192S8_RULE), L.GEMM_V_PIPE256S, (12, 47), 512)
    _is(_plan(_desc(144, 576), D | L.GEMM_MODE_KEEP_128WIDE), L.GEMM_V_WS96, (2, 125), 768)
    for kw in (DWIDE, dict(N=2048, K=512, **FFN_UP), dict(N=144, K=576)):
        assert _plan(_desc(**kw)).epilogue != L.GEMM_EPI_GENERIC
        assert _plan(_desc(**kw), D | L.GEMM_MODE_GENERIC_EPILOGUE).epilogue == L.GEMM_EPI_GENERIC
    # the CU count decides between 96- and 192-row warp-specialised tiles: 126 tiles of 192 rows * 5 <= 3 * cus
    _is(_plan(_desc(256, 1024), cus=209), L.GEMM_V_WS192, (2, 63))
    _is(_plan(_desc(256, 1024), cus=210), L.GEMM_V_WS96, (2, 125))


def test_forced_selectors_and_staged_mode():
    d = _desc(**DWIDE)
    _is(_plan(d, _forced(L.GEMM_SEL_PIPE256)), L.GEMM_V_PIPE256, (4, 47), 512, L.GEMM_EPI_GENERIC)
    _is(_plan(d, _forced(L.GEMM_SEL_PIPE256S)), L.GEMM_V_PIPE256S, (4, 47), 512, L.GEMM_EPI_F32_RES)
    _is(_plan(d, _forced(L.GEMM_SEL_192)), L.GEMM_V_WS192, (4, 63), 768, L.GEMM_EPI_F32_RES)
    _is(_plan(d, _forced(L.GEMM_SEL_PIPE192S8)), L.GEMM_V_PIPE192S8, (4, 63), 512, L.GEMM_EPI_F32_RES)
    assert _forced(L.GEMM_SEL_PIPE192S8) == 114 and D | L.GEMM_MODE_KEEP_WS192 == 3 | 8388608   # the integers scripts pass
    # a layout without the forced variant falls back to its own rule (MN-major A has no 192-row kernels)
    _is(_plan(_desc(512, 512, a_kmajor=0), _forced(L.GEMM_SEL_192)), L.GEMM_V_PIPE256S, (4, 47), 512)
    # mode 1: register-staged; 256-row tiles from 512 tiles on (47 x 16 = 752), else 128-row ones (47 x 4 = 188)
    _is(_plan(_desc(2048, 512), L.GEMM_MODE_STAGED256), L.GEMM_V_STAGED_BF16_256, (16, 47), 512, L.GEMM_EPI_GENERIC)
    _is(_plan(d, L.GEMM_MODE_STAGED256), L.GEMM_V_STAGED_BF16_128, (4, 94), 256, L.GEMM_EPI_GENERIC)
    _is(_plan(_desc(2048, 512), 0), L.GEMM_V_STAGED_BF16_128, (16, 94), 256)     # 256-row staged tiles not allowed


def test_other_layouts_and_fallbacks():
    _is(_plan(_desc(512, 2048, b_kmajor=0)), L.GEMM_V_PIPE192, (4, 63), 512, L.GEMM_EPI_GENERIC)   # K-major x MN-major
    _is(_plan(_desc(512, 512, a_kmajor=0)), L.GEMM_V_PIPE256S, (4, 47), 512, L.GEMM_EPI_GENERIC)   # MN-major A:
    _is(_plan(_desc(512, 1024, a_kmajor=0)), L.GEMM_V_PIPE256, (4, 47), 512)                       # k_per_split <= 512?
    _is(_plan(_desc(512, 1024, a_kmajor=0, b_kmajor=0)), L.GEMM_V_PIPE256, (4, 47), 512)
    _is(_plan(_desc(512, 512, lda=516)), L.GEMM_V_STAGED_BF16_128, (4, 94), 256)                    # lda % 8 != 0
    _is(_plan(_desc(512, 512, A=PA + 2)), L.GEMM_V_STAGED_BF16_128, (4, 94), 256)                   # A not 16-B aligned
    # split-K: plain fp32 epilogue, k_per_split = 512 -> two-per-CU 256-row tiles, z = the slices
    _is(_plan(_desc(512, 2048, dtype_c=F32, split_k=4)), L.GEMM_V_PIPE256S, (4, 47, 4), 512, L.GEMM_EPI_GENERIC)
    # fp32 operands: under 256 workgroups of 128 x 128 the 64-row kernel, else the 128-row one
    _is(_plan(_desc(512, 64, M=512, dt=F32, dtype_c=F32)), L.GEMM_V_STAGED_F32_64, (8, 8), 256, L.GEMM_EPI_GENERIC)
    _is(_plan(_desc(2048, 64, dt=F32, dtype_c=F32)), L.GEMM_V_STAGED_F32_128, (16, 94), 256)
    _is(_plan(_desc(0, 64)), L.GEMM_V_NONE)                                                          # empty output


def test_fp8_variants():
    mx = dict(dt=FP8, mx_a=PX, mx_b=PX + 4096)
    _is(_plan(_desc(512, 512, **mx)), L.GEMM_V_MX192, (4, 63), 512, L.GEMM_EPI_BF16)
    _is(_plan(_desc(2048, 2048, **mx)), L.GEMM_V_MX192, (16, 63), 512)
    _is(_plan(_desc(2048, 512, **mx)), L.GEMM_V_MX256S, (16, 47), 512)
    out = dict(mx_out=PX + 8192, mx_out_scales=PX + 12288)
    _is(_plan(_desc(2048, 512, **mx, **FFN_UP, **out)), L.GEMM_V_MX256S, (16, 47), 512, L.GEMM_EPI_BF16_SILU_MX)
    _is(_plan(_desc(512, 2048, dt=FP8)), L.GEMM_V_FP8_192, (4, 63), 512, L.GEMM_EPI_GENERIC)
    _is(_plan(_desc(2048, 512, dt=FP8)), L.GEMM_V_FP8_256S, (16, 47), 512, L.GEMM_EPI_GENERIC)


def test_plan_and_launch_return_the_same_errors():
    lib = L.load()
    mx = dict(dt=FP8, mx_a=PX, mx_b=PX + 4096, mx_out=PX + 8192, mx_out_scales=PX + 12288)
    cases = [(_desc(2048, 512, **mx), D, -5),                              # mx_out without the FFN-up epilogue
             (_desc(128, 64, M=128, batch=70000), D, -2),                  # grid too large, LDS-DMA path
             (_desc(128, 64, M=128, batch=70000), L.GEMM_MODE_STAGED256, -2),   # ... register-staged path
             (_desc(512, 512, dtype_c=BF16, split_k=2), D, -1)]            # split-K needs a plain fp32 epilogue
    for d, mode, want in cases:
        c = L.GemmChoice()
        assert lib.cfm_gemm_plan(ctypes.byref(d), mode, CUS, ctypes.byref(c)) == want
        msg = lib.cfm_get_last_error()
        lib.cfm_gemm_set_mode(mode)
        try:
            assert lib.cfm_gemm(ctypes.byref(d), None) == want     # rejected before any launch
        finally:
            lib.cfm_gemm_set_mode(D)
        assert lib.cfm_get_last_error() == msg
    # mode < 0: the current cfm_gemm_set_mode value; cus <= 0 and a null result are argument errors
    lib.cfm_gemm_set_mode(D | L.GEMM_MODE_KEEP_SHARED_DMA)
    try:
        _is(_plan(_desc(**DWIDE), -1), L.GEMM_V_PIPE192)
    finally:
        lib.cfm_gemm_set_mode(D)
    _is(_plan(_desc(**DWIDE), -1), L.GEMM_V_WS192)
    c = L.GemmChoice()
    assert lib.cfm_gemm_plan(ctypes.byref(_desc(**DWIDE)), D, 0, ctypes.byref(c)) == -1
    assert lib.cfm_gemm_plan(ctypes.byref(_desc(**DWIDE)), D, CUS, None) == -1


def _header_enum(name):
    """name -> value of every enumerator of `enum <name>` in cfm.h (comments stripped as the export test does)"""
    src = open(os.path.join(REPO, "include", "cfm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"enum\s+%s\s*\{(.*?)\}" % name, src, flags=re.S).group(1)
    out, nxt = {}, 0
    for item in filter(None, (s.strip() for s in body.split(","))):
        k, _, v = (s.strip() for s in item.partition("="))
        out[k] = eval(v, {}, dict(out)) if v else nxt
        nxt = out[k] + 1
    return out


@pytest.mark.parametrize("enum,cprefix,pyprefix", [
    ("cfm_gemm_mode", "CFM_GEMM_MODE_", "GEMM_MODE_"), ("cfm_gemm_sel", "CFM_GEMM_SEL_", "GEMM_SEL_"),
    ("cfm_gemm_variant", "CFM_GEMM_V_", "GEMM_V_"), ("cfm_gemm_epilogue", "CFM_GEMM_EPI_", "GEMM_EPI_"),
    ("cfm_attn_mode", "CFM_ATTN_MODE_", "ATTN_MODE_"), ("cfm_attn_path", "CFM_ATTN_PATH_", "ATTN_PATH_"),
    ("cfm_attn_dpos", "CFM_ATTN_DPOS_", "ATTN_DPOS_"), ("cfm_attn_ws", "CFM_ATTN_WS_", "ATTN_WS_")])
def test_python_constants_mirror_the_header(enum, cprefix, pyprefix):
    hdr = _header_enum(enum)
    assert len(hdr) >= (4 if enum in ("cfm_attn_path", "cfm_attn_dpos", "cfm_attn_ws") else 5)
    assert all(k.startswith(cprefix) for k in hdr)
    mirror = {cprefix + k[len(pyprefix):]: v for k, v in vars(L).items() if k.startswith(pyprefix) and isinstance(v, int)}
    assert mirror == hdr
    if enum == "cfm_gemm_mode":
        assert hdr["CFM_GEMM_MODE_DEFAULT"] == 3
