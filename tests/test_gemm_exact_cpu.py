"""The exact-GEMM table and helpers (tests/gemm_exact.py) checked without a GPU: every row's cfm_gemm_plan result is the
variant and epilogue kind the row names (cfm_gemm_plan is pure host arithmetic: test_gemm_plan_cpu.py), the table
covers every variant, epilogue kind, layout and leading-dimension form, the guard helpers catch a single changed byte,
and the premise of the GPU file -- fp32 sums of these integer products are exact in any order -- holds on the CPU for
every shape in the table."""
import ctypes

import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib as L
from nn_conformer_for_speech_recognition_amd import ops
from tests import gemm_exact as ge

CUS = 256


@pytest.mark.parametrize("case", ge.CASES, ids=[c.id for c in ge.CASES])
def test_row_launches_the_variant_and_epilogue_it_names(case):
    d = ops._gemm_desc(**ge.plan_fields(case))
    c = L.GemmChoice()
    rc = L.load().cfm_gemm_plan(ctypes.byref(d), ge.mode_value(case.mode), CUS, ctypes.byref(c))
    assert rc == 0, L.load().cfm_get_last_error()
    assert (c.variant, c.epilogue) == (case.variant, case.epilogue)
    # rules that read the CU count (96- vs 192-row warp-specialised tiles) must not decide a row: the GPU test plans
    # with the device's own count
    for cus in (64, 304):
        assert L.load().cfm_gemm_plan(ctypes.byref(d), ge.mode_value(case.mode), cus, ctypes.byref(c)) == 0
        assert (c.variant, c.epilogue) == (case.variant, case.epilogue), cus


def _enum(prefix):
    return {k: v for k, v in vars(L).items() if k.startswith(prefix) and isinstance(v, int)}


def test_table_covers_every_variant_epilogue_and_layout():
    variants = _enum("GEMM_V_")
    missing = {k for k, v in variants.items() if k != "GEMM_V_NONE" and v not in {c.variant for c in ge.CASES}}
    assert not missing, f"kernel variants without a row in tests/gemm_exact.py CASES: {sorted(missing)}"
    epis = _enum("GEMM_EPI_")
    missing = {k for k, v in epis.items() if v not in {c.epilogue for c in ge.CASES}}
    assert not missing, f"epilogue kinds without a row: {sorted(missing)}"
    assert {c.layout for c in ge.CASES} == {"kxk", "kxmn", "mnxk", "mnxmn"}
    assert any(c.split_k > 1 for c in ge.CASES) and any(c.batch > 1 for c in ge.CASES)
    assert any(c.a_kmajor and not c.overlap and c.lda > c.K for c in ge.CASES)
    assert any(c.b_kmajor and c.ldb > c.K for c in ge.CASES)
    assert any(c.ldc > c.N for c in ge.CASES)
    assert any(c.overlap and c.lda < c.K for c in ge.CASES)
    # every compile-time kind also runs through the generic rows, and every variant has a real-valued row
    for kind, (epi, _) in ge.EPILOGUES.items():
        assert any(c.id.endswith(kind) and c.epilogue == epi for c in ge.CASES), kind
        assert any(c.id.endswith(kind) and c.epilogue == L.GEMM_EPI_GENERIC and "generic" in c.mode for c in ge.CASES), kind
    bf16_f32 = {v for k, v in variants.items() if k != "GEMM_V_NONE" and "FP8" not in k and "MX" not in k}
    assert bf16_f32 <= {c.variant for c in ge.REAL_CASES}


ALL4 = ("kxk", "kxmn", "mnxk", "mnxmn")
# variant -> (tile height, the layouts it takes, whether it takes N % 8 != 0)
EDGES = {
    "STAGED_BF16_256": (256, ALL4, True), "STAGED_BF16_128": (128, ALL4, True),
    "STAGED_F32_128": (128, ALL4, True), "STAGED_F32_64": (64, ALL4, True),
    "PIPE64X160": (64, ("kxk",), False), "WS192": (192, ("kxk",), False), "WS96": (96, ("kxk",), False),
    "PIPE192": (192, ("kxk", "kxmn"), False), "PIPE192S8": (192, ("kxk", "kxmn"), False),
    "PIPE256": (256, ALL4, False), "PIPE256S": (256, ALL4, False),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_every_variant_has_its_edges_in_every_layout(name):
    """per bf16 / fp32 variant and per layout it takes, among the plain integer rows: M in {1, h - 1, h + 1, ragged
    against two tiles} (MN-major A: 8, h - 8, h + 8 -- M % 8 == 0 there), N in {one 8-chunk, a tile + 8, two tiles + 8}
    (the 160-wide tile: a ragged and a full tile, it takes N in 129..160 only) plus N % 8 != 0 where the variant takes
    it, K in {8, 64, 72, 144, 200, 1000}"""
    h, layouts, odd_n = EDGES[name]
    v = getattr(L, "GEMM_V_" + name)
    for lay in layouts:
        rows = [c for c in ge.INT_CASES if c.variant == v and c.layout == lay and not c.overlap and c.split_k == 1]
        ms, ns, ks = {c.M for c in rows}, {c.N for c in rows}, {c.K for c in rows}
        want_m = {1, h - 1, h + 1} if lay.startswith("k") else {8, h - 8, h + 8}
        assert want_m <= ms and any(m > h + 8 and m % h for m in ms), (name, lay, sorted(ms))
        want_n = {136, 160} if name == "PIPE64X160" else {8, 72 if name == "STAGED_F32_64" else 136}
        assert want_n <= ns and (name == "PIPE64X160" or any(n > 2 * (64 if name == "STAGED_F32_64" else 128) for n in ns)), \
            (name, lay, sorted(ns))
        assert not odd_n or {130, 77} <= ns, (name, lay, sorted(ns))
        assert {8, 64, 72, 144, 200, 1000} <= ks, (name, lay, sorted(ks))
        assert all(c.lda > (c.K if c.a_kmajor else c.M) and c.ldc > c.N for c in rows if "unaligned" not in c.id
                   and "tight" not in c.id and c.via == "gemm"), (name, lay)


def test_fp8_variants_have_the_rows_the_kernels_take():
    """fp8 / MX: K-major only, K % 128 == 0: K in {128, 640}, ragged M, N in {136, 520} as the selection allows (the
    two-per-CU tiles run for N > 512 only, MX256S also for K <= 512 only)"""
    for name, ns, ks in (("FP8_192", {136}, {128, 640}), ("FP8_256S", {520}, {128, 640}),
                         ("MX192", {136, 520}, {128, 640}), ("MX256S", {520}, {128})):
        rows = [c for c in ge.CASES if c.variant == getattr(L, "GEMM_V_" + name) and not c.mx_out]
        assert {c.N for c in rows} == ns and {c.K for c in rows} == ks and {c.M for c in rows} == {193, 385}, name


def test_fp64_reference_path_equals_int64():
    g = torch.Generator().manual_seed(11)
    A = ge.int_operand((70, 257, 1000), torch.bfloat16, g)
    B = ge.int_operand((136, 1000), torch.bfloat16, g)
    assert A.numel() // 1000 * B.numel() > 1 << 27          # the fp64 path
    assert torch.equal(ge.int_matmul(A, B), A.to(torch.int64) @ B.to(torch.int64).T)


def test_table_stays_small():
    for c in ge.CASES:
        fp8 = c.dtype_ab in ("fp8", "mx")
        # fp8 rows: N up to 520; the one MX256S mx_out row needs N > 512 with N % 32 == 0, of which 544 is the first
        assert c.M <= 520 and c.N <= ((544 if c.mx_out else 520) if fp8 else 330), c.id
        assert c.K <= 1000 or (c.K == 5000 and (c.M, c.N) == (256, 192) and c.split_k > 1), c.id


def test_int_operand_refuses_inexact_reductions():
    g = torch.Generator().manual_seed(0)
    x = ge.int_operand((3, 1000), torch.bfloat16, g)
    assert x.dtype == torch.bfloat16 and float(x.abs().max()) <= 4 and bool((x == x.round()).all())
    assert set(ge.int_operand((4096,), torch.float32, g).tolist()) == set(range(-4, 5))
    ge.int_operand((2, (1 << 20) - 1), torch.float32, g)                  # 16 K just below 2^24
    with pytest.raises(ValueError):
        ge.int_operand((2, 1 << 20), torch.float32, g)                    # 16 K = 2^24
    with pytest.raises(ValueError):
        ge.int_operand((2, 8), torch.float32, g, k=5000, fan_in=256)      # the rowdot fan-in counts
    ge.int_operand((2, 1 << 21), torch.float32, g, lo=-2, hi=2)           # a smaller range buys a longer K
    # e4m3 holds k * 64 for |k| <= 4 exactly (the device's power-of-two scaling of these operands)
    v = torch.arange(-4, 5, dtype=torch.float32) * 64
    assert torch.equal(v.to(torch.float8_e4m3fn).float(), v)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8])
@pytest.mark.parametrize("fill", ["sentinel", "nan"])
def test_guards_detect_a_single_changed_byte(dtype, fill):
    es = torch.empty(0, dtype=dtype).element_size()
    g = ge.guarded(5, 24, 32, dtype, fill, batch=2)
    buf, view = g
    assert view.shape == (2, 5, 24) and view.stride() == (5 * 32 + 64, 32, 1)
    assert g.first * es >= 64 << 10 and (buf.numel() - g.first - g.stride - g.span) * es >= 64 << 10
    if dtype in (torch.bfloat16, torch.float32):
        assert bool(torch.isnan(buf).all()) if fill == "nan" else bool((buf == ge.SENTINEL).all())
    ge.assert_untouched(g)
    g.set(torch.ones(2, 5, 24).to(dtype))                  # writing the logical matrix is no violation
    ge.assert_untouched(g)
    raw = g.rawbuf.view(torch.uint8)
    spots = {"guard before": 3, "last guard byte": raw.numel() - 1, "byte before the first element": g.first * es - 1,
             "padding column": (g.first + 24) * es, "last padding column of a row": (g.first + 2 * 32 - 1) * es + es - 1,
             "gap between batches": (g.first + 5 * 32 + 7) * es, "after the last element": (g.first + g.stride + g.span) * es}
    for what, at in spots.items():
        raw[at] ^= 1
        with pytest.raises(AssertionError, match="outside the logical"):
            ge.assert_untouched(g, what)
        raw[at] ^= 1
        ge.assert_untouched(g, what)
    # the reported offset is relative to the first logical element
    raw[(g.first + 24) * es] ^= 1
    with pytest.raises(AssertionError, match=r"\[24\]"):
        ge.assert_untouched(g)


def test_guarded_overlapping_rows_and_mask():
    g = ge.guarded(4, 10, 3, torch.float32, "nan")       # ld < cols: rows are windows of one run of 19 elements
    assert g.overlap and g.flat.numel() == 19
    g.flat.copy_(torch.arange(19.0))
    assert torch.equal(g.view[0], torch.arange(19.0).unfold(0, 10, 3))
    assert int(g.logical_mask().sum()) == 19
    m = ge.guarded(3, 5, 8, torch.bfloat16, "sentinel", batch=2).logical_mask()
    assert int(m.sum()) == 2 * 3 * 5
    ge.assert_untouched(g)


SHAPES = sorted({(c.M, c.N, c.K, c.lo, c.hi) for c in ge.INT_CASES})


def test_fp32_sums_in_any_order_equal_the_integer_reference():
    """the premise: for every shape of the table the int64 product, an fp32 matmul, one over a shuffled K order and a
    64-chunked one agree exactly; and the bf16 cast really rounds (elements change under it at K 1000)"""
    g = torch.Generator().manual_seed(5)
    changed = 0.0
    for M, N, K, lo, hi in SHAPES:
        A = ge.int_operand((M, K), torch.float32, g, lo, hi)
        B = ge.int_operand((N, K), torch.float32, g, lo, hi)
        ref = ge.int_matmul(A, B)
        assert int(ref.abs().max()) < ge.EXACT_LIMIT
        perm = torch.randperm(K, generator=g)
        chunked = sum(A[:, k:k + 64] @ B[:, k:k + 64].T for k in range(0, K, 64))
        for name, got in (("fp32", A @ B.T), ("shuffled", A[:, perm] @ B[:, perm].T), ("chunked", chunked)):
            assert torch.equal(got.to(torch.int64), ref) and got.dtype == torch.float32, (name, M, N, K)
        if K == 1000 and (lo, hi) == (-4, 4):
            r = ref.float()
            changed = max(changed, float((r.to(torch.bfloat16).float() != r).float().mean()))
    assert changed > 0.05, changed
