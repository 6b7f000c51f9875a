"""Exact element-wise GEMM checks: operands for which the exact answer is the only right answer, and buffers that show
what a kernel reads or writes outside its matrices (helpers of tests/test_gpu_gemm_exact.py and test_gemm_exact_cpu.py).

Operands are small integers (int_operand, [-4, 4] by default): exact in bf16, fp32 and -- after the device's power-of-two
scaling -- e4m3.  Every product is an integer of magnitude <= 16 and every partial sum, in any order, over any split-K
slicing and in any MFMA shape, an integer below 16 K; for 16 K < 2^24 fp32 accumulation is exact whatever the order, so
an fp32 output must EQUAL the int64 reference and a bf16 output its round-to-nearest-even cast, bit for bit.  alpha and
out_scale in {0.5, 1, 2}, integer bias / residual, the bias-gradient column sums and attention's rowdot keep that
property (powers of two and integer sums).

Every matrix lives inside a larger buffer (guarded): >= 64 KiB before the first and after the last element, plus the
ld > cols padding columns and the gaps between batches.  Outputs carry a finite sentinel there and assert_untouched
compares those positions' raw bits afterwards; inputs carry NaN there -- memory outside the logical extent of an operand
must not influence the result, whatever it holds (a clamped row or a zero-filled K tail never lets the NaN reach a
stored element; a kernel that reads real memory past K and relies on the other operand's zero does: NaN * 0 = NaN).

CASES is the table of cfm_gemm launches (pure data): shape, layouts, leading dimensions, dtypes, epilogue ingredients,
the cfm_gemm_set_mode value (by name, MODES) and the variant / epilogue kind the row must launch.  test_gemm_exact_cpu.py
pins every row's cfm_gemm_plan result and the table's coverage without a GPU."""
import contextlib
import ctypes
import dataclasses

import numpy as np
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ops

BF, F32, F8, U8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8
DTYPES = {"bf16": BF, "f32": F32}
EXACT_LIMIT = 1 << 24            # integers below 2^24 in magnitude are exact in fp32
GUARD_BYTES = 64 << 10
SENTINEL = -3.0
# raw bits of the guard / padding fill: NaN for inputs (e4m3fn: 0x7F, e8m0 scale bytes: 0xFF), -3.0 for outputs
# (e4m3: 0xC4; scale bytes: an arbitrary 0xA5)
_PATTERN = {("nan", BF): 0x7FC0, ("nan", F32): 0x7FC00000, ("nan", F8): 0x7F, ("nan", U8): 0xFF,
            ("sentinel", BF): 0xC040, ("sentinel", F32): 0xC0400000, ("sentinel", F8): 0xC4, ("sentinel", U8): 0xA5}
_BITS = {BF: torch.int16, F32: torch.int32, F8: torch.uint8, U8: torch.uint8}


# ------------------------------------------------------------------------------------------ launches under a plan probe
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def planned():
    """collects (variant, epilogue) of every ops.gemm launch in the block: cfm_gemm_plan on the very descriptor, under
    the current cfm_gemm_set_mode value, before it is launched"""
    seen = []
    n = cus()

    def probe(kind, shape, desc, launch):
        if kind == "gemm":
            c = _lib.GemmChoice()
            rc = _lib.load().cfm_gemm_plan(ctypes.byref(desc), -1, n, ctypes.byref(c))
            assert rc == 0, _lib.load().cfm_get_last_error()
            seen.append((c.variant, c.epilogue))
        return launch()
    ops.PROBE = probe
    try:
        yield seen
    finally:
        ops.PROBE = None


def gemm_mode_fixture():
    """body of the gemm_mode fixture: a setter for cfm_gemm_set_mode; the default mode is restored after the test"""
    yield lambda m: _lib.call("cfm_gemm_set_mode", m)
    _lib.call("cfm_gemm_set_mode", _lib.GEMM_MODE_DEFAULT)


# ------------------------------------------------------------------------------------------ operands and guarded buffers
def int_operand(shape, dtype, gen, lo=-4, hi=4, *, k=None, fan_in=1):
    """Integers uniform in [lo, hi] as a CPU tensor of `dtype`.  k: the reduction length the operand enters (default:
    its last dimension); fan_in: what multiplies a reduced value further before it is stored (a residual scale, the
    rowdot's 64 columns x |with|).  Raises when max|product| * k * fan_in reaches 2^24: exactness not guaranteed."""
    k = shape[-1] if k is None else k
    amax = max(abs(lo), abs(hi))
    if amax * amax * k * fan_in >= EXACT_LIMIT:
        raise ValueError(f"int_operand: {amax * amax} * K {k} * fan-in {fan_in} >= 2^24, fp32 sums would not be exact")
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(dtype)


def _signed(pattern, bits):
    width = torch.iinfo(bits).bits
    return pattern - (1 << width) if bits != torch.uint8 and pattern >= 1 << (width - 1) else pattern


class Guarded:
    """A logical (batch, rows, cols) matrix with row stride ld and batch stride `stride` (elements) inside a buffer
    filled with a guard pattern.  buf: the whole 1-D buffer; view: the logical matrix (a strided view of buf; with
    ld < cols -- overlapping rows, one batch -- write through `flat`, the (rows - 1) ld + cols elements it spans);
    bits: view as raw integers."""

    def __init__(self, rows, cols, ld, dtype, fill, batch=1, stride=None, device="cpu"):
        assert fill in ("nan", "sentinel") and rows >= 1 and cols >= 1 and ld >= 1 and batch >= 1
        es = torch.empty(0, dtype=dtype).element_size()
        self.rows, self.cols, self.ld, self.batch, self.dtype, self.fill = rows, cols, ld, batch, dtype, fill
        self.overlap = ld < cols
        assert not self.overlap or batch == 1
        self.span = (rows - 1) * ld + cols
        # default batch stride: whole rows plus a 64-element gap (keeps 16-byte alignment of every batch)
        self.stride = (rows * ld + 64 if stride is None else stride) if batch > 1 else 0
        assert batch == 1 or self.stride >= self.span
        self.first = GUARD_BYTES // es
        total = self.first + (batch - 1) * self.stride + self.span + GUARD_BYTES // es
        self.pattern = _PATTERN[fill, dtype]
        ib = _BITS[dtype]
        self.rawbuf = torch.full((total,), _signed(self.pattern, ib), dtype=ib, device=device)
        self.buf = self.rawbuf.view(dtype)
        size, strides = (batch, rows, cols), (self.stride, ld, 1)
        self.view = torch.as_strided(self.buf, size, strides, self.first)
        self.bits = torch.as_strided(self.rawbuf, size, strides, self.first)
        self.flat = self.buf[self.first:self.first + self.span] if batch == 1 else None

    def __iter__(self):          # buf, view = guarded(...)
        return iter((self.buf, self.view))

    def set(self, values):
        """values: (batch, rows, cols) or (rows, cols) of this dtype (any device)"""
        assert not self.overlap
        v = values.reshape(self.batch, self.rows, self.cols)
        if self.dtype in (F8, U8):
            self.bits.copy_(v.contiguous().view(torch.uint8))
        else:
            self.view.copy_(v)
        return self

    def poison(self):
        """an output's logical region filled with NaN (fp8: 0x7F, scale bytes: 0xFF), so an element no thread stores
        fails the comparison whatever its expected value"""
        assert not self.overlap
        self.bits.fill_(_signed(_PATTERN["nan", self.dtype], self.rawbuf.dtype))
        return self

    def logical_mask(self):
        """numpy bool over buf: True at the positions of the logical matrix"""
        m = np.zeros(self.rawbuf.numel(), dtype=bool)
        if self.overlap:
            m[self.first:self.first + self.span] = True
            return m
        rows = self.first + (np.arange(self.batch)[:, None] * self.stride + np.arange(self.rows)[None, :] * self.ld)
        m[(rows.reshape(-1, 1) + np.arange(self.cols)[None, :]).reshape(-1)] = True
        return m


def guarded(rows, cols, ld, dtype, fill, batch=1, stride=None, device="cpu"):
    """-> Guarded (unpacks as (buffer, logical view)): fill "sentinel" for outputs, "nan" for inputs"""
    return Guarded(rows, cols, ld, dtype, fill, batch, stride, device)


def assert_untouched(g, what=""):
    """every guard, padding and inter-batch position of g still holds the fill pattern, bit for bit"""
    bits = g.rawbuf.cpu().numpy()
    want = np.array(_signed(g.pattern, g.rawbuf.dtype)).astype(bits.dtype)
    bad = np.flatnonzero(~g.logical_mask() & (bits != want))
    assert bad.size == 0, (f"{what}: {bad.size} element(s) outside the logical {g.batch} x {g.rows} x {g.cols} (ld {g.ld}) "
                           f"matrix written; first offsets relative to its first element: {(bad[:6] - g.first).tolist()}")


def int_matmul(A, B):
    """int64 reference of sum_k A[.., m, k] B[n, k] (A (.., M, K), B (N, K) logical K-major tensors of any dtype).
    Large batched products run through the fp64 BLAS: every partial sum is an integer far below 2^53, so that is the
    same number (test_gemm_exact_cpu.py holds the two paths to each other)."""
    if A.numel() // A.shape[-1] * B.numel() > 1 << 27:
        return (A.double() @ B.double().transpose(-1, -2)).to(torch.int64)
    return A.to(torch.int64) @ B.to(torch.int64).transpose(-1, -2)


def first_mismatches(got, want, n=4):
    """'(index) got want' of the first n differing elements, for assertion messages"""
    bad = (got != want) | (got != got)
    idx = bad.nonzero()[:n]
    return [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx], int(bad.sum())


# ------------------------------------------------------------------------------------------ the table
def forced(sel):
    """the mode word that forces one bf16 pipeline variant (CFM_GEMM_SEL_*)"""
    return _lib.GEMM_MODE_PIPE | sel << _lib.GEMM_MODE_SEL_SHIFT


# the cfm_gemm_set_mode values the suite forces kernels with (test_gpu_dropout_masks.MODES takes them from here);
# "<name>+generic" adds GEMM_MODE_GENERIC_EPILOGUE
MODES = {
    "default": _lib.GEMM_MODE_DEFAULT,
    "staged": _lib.GEMM_MODE_STAGED256,
    "pipe256": forced(_lib.GEMM_SEL_PIPE256),
    "pipe256s": forced(_lib.GEMM_SEL_PIPE256S),
    "ws96": forced(_lib.GEMM_SEL_192),
    "ws192": forced(_lib.GEMM_SEL_192) | _lib.GEMM_MODE_KEEP_WS192,
    "pipe192": forced(_lib.GEMM_SEL_192) | _lib.GEMM_MODE_KEEP_SHARED_DMA,
    "pipe192s8": forced(_lib.GEMM_SEL_PIPE192S8),
}


def mode_value(name):
    base, _, extra = name.partition("+")
    assert extra in ("", "generic")
    return MODES[base] | (_lib.GEMM_MODE_GENERIC_EPILOGUE if extra else 0)


@dataclasses.dataclass(frozen=True)
class Case:
    """One cfm_gemm launch.  M, N, K: the GEMM's (via "linear_wgrad": ops.linear_wgrad(dy (K, M), x (K, N)) launches
    it).  dtype_ab: bf16 | f32 | fp8 (per-tensor scales) | mx.  pre / residual: None or the tensor's dtype name;
    real: randn operands held to the derived forward bound instead of integers held to equality."""
    id: str
    mode: str
    M: int
    N: int
    K: int
    variant: int
    epilogue: int
    a_kmajor: bool = True
    b_kmajor: bool = True
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    dtype_ab: str = "bf16"
    dtype_c: str = "bf16"
    alpha: float = 1.0
    bias: bool = False
    act: bool = False
    act_grad: bool = False
    pre: str = None
    out_scale: float = 1.0
    residual: str = None
    rowdot: int = 0              # rowdot_T (0: off)
    mx_out: bool = False
    split_k: int = 1
    batch: int = 1
    overlap: bool = False
    atomic: bool = False         # split_k > 1 without a workspace: partial sums added into a zeroed C
    via: str = "gemm"
    lo: int = -4
    hi: int = 4
    real: bool = False

    @property
    def layout(self):
        return ("k" if self.a_kmajor else "mn") + "x" + ("k" if self.b_kmajor else "mn")


V = _lib
G = _lib.GEMM_EPI_GENERIC
# variants whose K-major x K-major launches carry the compile-time epilogue kinds
_CARRY = {V.GEMM_V_PIPE64X160, V.GEMM_V_WS192, V.GEMM_V_WS96, V.GEMM_V_PIPE192S8, V.GEMM_V_PIPE256S}
KK, KMN, MNK, MNMN = (True, True), (True, False), (False, True), (False, False)
_LNAME = {KK: "kk", KMN: "kmn", MNK: "mnk", MNMN: "mnmn"}


def _case(mode, variant, M, N, K, lay=KK, *, pad=(8, 16, 8), epi=None, tag="", **kw):
    ak, bk = lay
    dt = kw.get("dtype_ab", "bf16")
    lda = kw.pop("lda", None) or (K if ak else M) + pad[0]
    ldb = kw.pop("ldb", None) or (K if bk else N) + pad[1]
    ldc = kw.pop("ldc", None) or N + pad[2]
    if epi is None:          # a plain store of the C dtype
        fast = variant in _CARRY and ak and bk and N % 8 == 0 and ldc % 8 == 0 and "generic" not in mode
        plain = _lib.GEMM_EPI_BF16 if kw.get("dtype_c", "bf16") == "bf16" else _lib.GEMM_EPI_F32
        epi = plain if fast and dt == "bf16" else G
    name = f"{mode}-{_LNAME[lay]}-{M}x{N}x{K}" + ("" if dt == "bf16" else f"-{dt}")
    name += (f"-b{kw['batch']}" if kw.get("batch", 1) > 1 else "") + (f"-{tag}" if tag else "")
    return Case(id=name, mode=mode, M=M, N=N, K=K, variant=variant, epilogue=epi, a_kmajor=ak, b_kmajor=bk, lda=lda,
                ldb=ldb, ldc=ldc, **kw)


def _sweep(mode, variant, h, lay, *, wide=128, ns=None, ks=None, ms=None, tiles=None, **kw):
    """the M, N and K edges of one variant in one layout, one dimension at a time: M in {1, h - 1, h + 1, ragged
    against two tiles} (MN-major A: multiples of 8) at N = wide + 8, K = 72; N in {8, wide + 8, two tiles + 8} at
    M = h + 1, K = 144; K in {8, one tile, the 8-multiple tails 72 / 144 / 200, 1000 -- every ring stage wraps} at
    M = h + 1, N = wide + 8.  lda = K + 8, ldb = K + 16, ldc = N + 8 throughout.  tiles = (bm, bn, count): the variant
    is selected from `count` bm x bn tiles on, so every row is batched just far enough to reach it (B shared)."""
    ak, bk = lay
    if ms is None:
        ms = [1, h - 1, h + 1, 97 if h == 64 else 385] if ak else [8, h - 8, h + 8, 104 if h == 64 else 392]
    ns = ns or [8, wide + 8, 2 * wide + 8]
    ks = ks or [8, 64, 72, 144, 200, 1000]
    n1 = wide + 8 if wide + 8 in ns else ns[0]
    m1 = h + 1 if ak else h + 8

    def row(m, n, k):
        if tiles is None:
            return _case(mode, variant, m, n, k, lay, **kw)
        bm, bn, count = tiles
        per = -(-m // bm) * -(-n // bn)
        return _case(mode, variant, m, n, k, lay, batch=-(-count // per), **kw)
    out = [row(m, n1, 72) for m in ms]
    out += [row(m1, n, 144) for n in ns if n != n1]
    out += [row(m1, n1, k) for k in ks if k != 72]
    return out


# epilogue ingredients by kind: (compile-time kind, fields).  SiLU rows use operands in [-1, 1] with K <= 72, so
# |pre| <= 73 and silu(pre) stays a normal number in fp32 and bf16 (x e^x underflows below x ~ -87).
# SiLU rows with an fp32 C use K = 8 (|pre| <= 9): the device forms e^-x as exp2(-x log2 e), and the fp32 rounding of
# that product alone (half an ulp of an argument of size |x| log2 e) is a relative error of up to |x| 2^-24 in e^-x,
# which silu(x) ~ x e^x inherits for x << 0; with one ulp each for v_exp_f32, v_rcp_f32 and the two other roundings
# the total is about (|x| + 6) 6e-8, inside the 2^-23 + 2e-6 of the comparison only for |x| below ~29 -- a bound K = 72
# does not give.  (A bf16 C rounds by 2^-8, far above this, so those rows keep K = 72.)
SILU_F32_K = 8
_S = dict(lo=-1, hi=1)
EPILOGUES = {
    "bf16": (V.GEMM_EPI_BF16, dict()),
    "bf16_bias": (V.GEMM_EPI_BF16_BIAS, dict(bias=True)),
    "bf16_silu": (V.GEMM_EPI_BF16_SILU, dict(bias=True, act=True, pre="bf16", **_S)),
    "bf16_actg": (V.GEMM_EPI_BF16_ACTG, dict(act_grad=True, pre="bf16")),
    "bf16_rd": (V.GEMM_EPI_BF16_RD, dict(rowdot=1)),
    "f32": (V.GEMM_EPI_F32, dict(dtype_c="f32", alpha=2.0, bias=True, out_scale=0.5)),
    "f32_silu": (V.GEMM_EPI_F32, dict(dtype_c="f32", bias=True, act=True, pre="bf16", **_S)),
    "f32_res": (V.GEMM_EPI_F32_RES, dict(dtype_c="f32", bias=True, out_scale=0.5, residual="f32")),
    "bf16_res": (V.GEMM_EPI_BF16_RES, dict(bias=True, out_scale=2.0, residual="bf16")),
    "f32r_bf16": (V.GEMM_EPI_F32R_BF16, dict(bias=True, out_scale=0.5, residual="f32")),
    "bf16_delta": (V.GEMM_EPI_BF16_DELTA, dict(bias=True, out_scale=0.5)),
}


def _epilogue_rows(mode, variant, M, N, K):
    """every compile-time kind on one carrying variant, and the same ingredients through the generic rows"""
    out = []
    for kind, (epi, f) in EPILOGUES.items():
        n = 192 if f.get("rowdot") and N % 64 else N
        if f.get("rowdot") and variant == V.GEMM_V_PIPE64X160:
            continue                                # no 64-column multiple in 129..160
        f = dict(f)
        if f.get("rowdot"):
            f["rowdot"] = M // 5 if M % 5 == 0 else M        # 5 "utterances" where M allows
        k = SILU_F32_K if kind == "f32_silu" else 72 if f.get("act") else K
        for md, e in ((mode, epi), (mode + "+generic", G)):
            out.append(_case(md, variant, M, n, k, KK, epi=e, tag=kind, **f))
    return out


def _build():
    c = []
    s = _sweep
    # ---- register-staged bf16, 128-row tiles: every layout, and N that is no multiple of 8
    for lay in (KK, KMN, MNK, MNMN):
        c += s("staged", V.GEMM_V_STAGED_BF16_128, 128, lay, ns=[8, 136, 264, 130, 77])
    c += [_case("staged", V.GEMM_V_STAGED_BF16_128, 129, 77, 72, KK, pad=(3, 5, 0), tag="unaligned"),
          _case("staged", V.GEMM_V_STAGED_BF16_128, 127, 130, 37, MNMN, pad=(1, 1, 1), tag="unaligned")]
    # MN-major operands whose M / N is no multiple of 8, and an unaligned lda: the LDS-DMA modes fall back to staged
    c += [_case("pipe256s", V.GEMM_V_STAGED_BF16_128, 97, 136, 72, MNK, tag="fallback"),
          _case("default", V.GEMM_V_STAGED_BF16_128, 129, 130, 72, KMN, tag="fallback"),
          _case("ws96", V.GEMM_V_STAGED_BF16_128, 97, 136, 72, KK, pad=(4, 16, 8), tag="fallback")]
    # ---- register-staged bf16, 256-row tiles: selected from 512 tiles of 256 x 128 on, so every row is batched
    for lay in (KK, KMN, MNK, MNMN):
        c += s("staged", V.GEMM_V_STAGED_BF16_256, 256, lay, ns=[8, 136, 264, 130, 77], tiles=(256, 128, 512))
    # ---- register-staged fp32 (exact-f32 MFMA): 64-row tiles under 256 workgroups, 128-row tiles from there on
    f32 = dict(dtype_ab="f32", dtype_c="f32")
    for lay in (KK, KMN, MNK, MNMN):
        c += s("default", V.GEMM_V_STAGED_F32_64, 64, lay, wide=64, ns=[8, 72, 136, 130, 77], **f32)
    c += [_case("default", V.GEMM_V_STAGED_F32_64, 65, 77, 37, KK, pad=(1, 3, 0), tag="unaligned", **f32),
          _case("default", V.GEMM_V_STAGED_F32_128, 257, 264, 200, MNMN, batch=29, **f32)]
    for lay in (KK, KMN, MNK, MNMN):     # 128-row fp32 tiles: from 256 workgroups of 128 x 128 on, so batched
        c += s("default", V.GEMM_V_STAGED_F32_128, 128, lay, ns=[8, 136, 264, 130, 77], tiles=(128, 128, 256), **f32)
    # ---- LDS-DMA pipeline and warp-specialised kernels (the 64 x 160 tile is selected for N in 129..160 only, always
    # one column tile: a ragged one, 136, and a full one, 160 -- tile width + 8 = 168 would launch another variant)
    c += s("default", V.GEMM_V_PIPE64X160, 64, KK, wide=160, ns=[136, 160], ms=[1, 63, 65, 97, 385])
    c += s("ws96", V.GEMM_V_WS96, 96, KK)
    c += s("ws192", V.GEMM_V_WS192, 192, KK)
    for lay in (KK, KMN):
        c += s("pipe192", V.GEMM_V_PIPE192, 192, lay)
        c += s("pipe192s8", V.GEMM_V_PIPE192S8, 192, lay)
    for lay in (KK, KMN, MNK, MNMN):
        c += s("pipe256", V.GEMM_V_PIPE256, 256, lay)
        c += s("pipe256s", V.GEMM_V_PIPE256S, 256, lay)
    c += [_case("pipe256s", V.GEMM_V_PIPE256S, 264, 136, 37, MNMN), _case("pipe256", V.GEMM_V_PIPE256, 264, 136, 37, MNMN)]
    # tight leading dimensions (the encoder's), default selection: K <= 512 two-per-CU, else BK 64
    c += [_case("default", V.GEMM_V_PIPE256S, 385, 264, 200, KK, pad=(0, 0, 0), tag="tight"),
          _case("default", V.GEMM_V_PIPE256, 257, 264, 1000, KMN, pad=(0, 0, 0), tag="tight")]
    # ---- every compile-time epilogue kind on every variant that carries them, and through the generic rows
    c += _epilogue_rows("default", V.GEMM_V_PIPE256S, 385, 264, 200)
    c += _epilogue_rows("default", V.GEMM_V_PIPE64X160, 97, 136, 200)
    c += _epilogue_rows("ws96", V.GEMM_V_WS96, 385, 264, 200)
    c += _epilogue_rows("ws192", V.GEMM_V_WS192, 385, 264, 200)
    c += _epilogue_rows("pipe192s8", V.GEMM_V_PIPE192S8, 385, 264, 200)
    # the generic-only kernels and the staged ones with a full epilogue; fp32 pre-activation (the parity mode)
    res = dict(dtype_c="f32", bias=True, out_scale=0.5, residual="f32")
    c += [_case("pipe192", V.GEMM_V_PIPE192, 385, 264, 200, KK, tag="f32_res", **res),
          _case("pipe256", V.GEMM_V_PIPE256, 385, 264, 200, KK, tag="f32_res", **res),
          _case("staged", V.GEMM_V_STAGED_BF16_128, 385, 130, 200, KK, tag="f32_res", **res),
          _case("staged", V.GEMM_V_STAGED_BF16_128, 129, 136, 72, KK, tag="silu", bias=True, act=True, pre="bf16", **_S),
          _case("default", V.GEMM_V_STAGED_F32_64, 65, 77, 8, KK, tag="silu_f32pre", bias=True, act=True, pre="f32",
                **_S, **f32),
          _case("default", V.GEMM_V_STAGED_F32_64, 65, 72, 72, KK, tag="actg_f32pre", act_grad=True, pre="f32", **f32),
          _case("default", V.GEMM_V_PIPE256S, 385, 264, 8, KK, epi=G, tag="silu_f32pre", bias=True, act=True,
                pre="f32", dtype_c="f32", **_S)]
    # ---- batch with stride_a, stride_c and gaps between the batches; the residual follows stride_c
    c += [_case("default", V.GEMM_V_PIPE256S, 193, 264, 200, KK, epi=V.GEMM_EPI_F32_RES, batch=3, tag="batch", **res),
          _case("ws96", V.GEMM_V_WS96, 97, 264, 144, KK, batch=3, tag="batch"),
          _case("pipe256", V.GEMM_V_PIPE256, 264, 136, 72, MNMN, batch=2, tag="batch")]
    # ---- overlapping A rows (lda < K, allow_overlap): the front-end fold's windowed view
    c += [_case("ws96", V.GEMM_V_WS96, 193, 136, 200, KK, lda=64, overlap=True, tag="overlap"),
          _case("default", V.GEMM_V_PIPE256S, 257, 264, 144, KK, lda=40, overlap=True, tag="overlap"),
          _case("staged", V.GEMM_V_STAGED_BF16_128, 129, 136, 72, KK, lda=24, overlap=True, tag="overlap")]
    # ---- split-K through linear_wgrad with bias_out (dW = dy^T x: MN-major x MN-major, K = the tokens; slabs and
    # the a_colsum bias gradient from split 2 on)
    wg = dict(via="linear_wgrad", dtype_c="f32", pad=(0, 0, 0))
    for M, N, K, split, v in [(136, 72, 1000, 1, V.GEMM_V_PIPE256), (136, 72, 1000, 4, V.GEMM_V_PIPE256S),
                              (264, 136, 1000, 8, V.GEMM_V_PIPE256S), (256, 192, 5000, 8, V.GEMM_V_PIPE256),
                              (136, 72, 200, 8, V.GEMM_V_PIPE256S)]:      # K 200 / 8: the last slices are empty
        c.append(_case("default", v, M, N, K, MNMN, split_k=split, tag=f"split{split}", **wg))
    # split-K of a plain cfm_gemm call: slabs in a workspace, or (atomic) sums added into a zeroed C; K-major operands
    # need whole 64-deep tiles per slice (K % 64 == 0), else the staged kernels run it
    sk = dict(dtype_c="f32", epi=G, bias=True)
    c += [_case("default", V.GEMM_V_PIPE256S, 257, 136, 960, KK, split_k=4, tag="split4", **sk),
          _case("default", V.GEMM_V_PIPE256S, 257, 136, 960, KK, split_k=4, atomic=True, tag="split4_atomic", **sk),
          _case("default", V.GEMM_V_STAGED_BF16_128, 129, 136, 1000, KK, split_k=4, tag="split4", **sk),
          _case("staged", V.GEMM_V_STAGED_BF16_128, 129, 130, 1000, MNMN, split_k=8, atomic=True, tag="split8_atomic", **sk),
          _case("default", V.GEMM_V_STAGED_F32_64, 65, 72, 200, KK, split_k=4, tag="split4", dtype_ab="f32", **sk)]
    # ---- fp8 e4m3, per-tensor scales (generic epilogue) and MX block scales; rows 16-byte aligned
    for kind, n_small, v_small, v_wide in (("fp8", 136, V.GEMM_V_FP8_192, V.GEMM_V_FP8_256S),
                                           ("mx", 136, V.GEMM_V_MX192, V.GEMM_V_MX256S)):
        e = G if kind == "fp8" else V.GEMM_EPI_BF16
        for M in (193, 385):
            for K in (128, 640):
                c.append(_case("default", v_small, M, n_small, K, KK, pad=(16, 32, 8), epi=e, dtype_ab=kind))
                wide = v_small if kind == "mx" and K > 512 else v_wide      # MX scale rows of K > 512: one per CU
                c.append(_case("default", wide, M, 520, K, KK, pad=(16, 32, 8), epi=e, dtype_ab=kind))
    mxo = dict(dtype_ab="mx", epi=V.GEMM_EPI_BF16_SILU_MX, bias=True, act=True, pre="bf16", mx_out=True,
               pad=(16, 32, 0), tag="mx_out", **_S)
    # (mx_out needs N % 32 == 0, and the two-per-CU MX kernel N > 512: 544 is the first such N, past the 520 of the
    # other fp8 rows)
    c += [_case("default", V.GEMM_V_MX192, 193, 160, 128, KK, **mxo), _case("default", V.GEMM_V_MX256S, 257, 544, 128, KK, **mxo)]
    # ---- one real-valued launch per variant (randn operands, the derived forward bound)
    real = dict(real=True, bias=True, tag="real")
    bb = V.GEMM_EPI_BF16_BIAS
    for mode, v, e in (("staged", V.GEMM_V_STAGED_BF16_128, G), ("ws96", V.GEMM_V_WS96, bb), ("ws192", V.GEMM_V_WS192, bb),
                       ("pipe192", V.GEMM_V_PIPE192, G), ("pipe192s8", V.GEMM_V_PIPE192S8, bb),
                       ("pipe256", V.GEMM_V_PIPE256, G), ("pipe256s", V.GEMM_V_PIPE256S, bb)):
        c.append(_case(mode, v, 385, 264, 200, KK, epi=e, **real))
    c += [_case("default", V.GEMM_V_PIPE64X160, 385, 152, 200, KK, epi=bb, **real),
          _case("staged", V.GEMM_V_STAGED_BF16_256, 385, 264, 200, KK, epi=G, batch=86, **real),
          _case("default", V.GEMM_V_STAGED_F32_64, 385, 264, 200, KK, epi=G, **real, **f32),
          _case("default", V.GEMM_V_STAGED_F32_128, 385, 264, 200, KK, epi=G, batch=22, **real, **f32),
          _case("pipe256s", V.GEMM_V_PIPE256S, 392, 264, 200, MNMN, epi=G, **real)]
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return c


CASES = _build()
INT_CASES = [c for c in CASES if not c.real]
REAL_CASES = [c for c in CASES if c.real]

# fake 4096-aligned pointers for cfm_gemm_plan (never dereferenced)
_PA, _PB, _PC, _PX = 1 << 20, 2 << 20, 3 << 20, 4 << 20


def plan_fields(case):
    """the cfm_gemm_desc fields of the row's launch with fake aligned pointers (cfm_gemm_plan reads only the values and
    alignment of pointers): what test_gpu_gemm_exact launches, minus the addresses"""
    fp8 = case.dtype_ab in ("fp8", "mx")
    px = iter(range(_PX, _PX + (1 << 20), 4096))
    f = dict(M=case.M, N=case.N, K=case.K, batch=case.batch,
             dtype_ab=_lib.FP8 if fp8 else _lib.dt(torch.empty(0, dtype=DTYPES[case.dtype_ab])),
             A=_PA, lda=case.lda, a_kmajor=int(case.a_kmajor), B=_PB, ldb=case.ldb, b_kmajor=int(case.b_kmajor),
             C=_PC, ldc=case.ldc, dtype_c=_lib.BF16 if case.dtype_c == "bf16" else _lib.F32, alpha=case.alpha,
             out_scale=case.out_scale, ldr=case.N, split_k=case.split_k, allow_overlap=int(case.overlap))
    if case.batch > 1:
        rows_a = case.M if case.a_kmajor else case.K
        f.update(stride_a=rows_a * case.lda + 64, stride_b=0, stride_c=case.M * case.ldc + 64)
    if case.bias:
        f["bias"] = next(px)
    if case.act:
        f["act"] = _lib.ACT_SILU
    if case.act_grad:
        f["act_grad"] = 1
    if case.pre:
        f.update(pre=next(px), dtype_pre=_lib.BF16 if case.pre == "bf16" else _lib.F32)
    if case.residual:
        f.update(residual=next(px), ldr=case.ldc if case.batch > 1 else case.N + 16,
                 dtype_r=_lib.BF16 if case.residual == "bf16" else _lib.F32)
    if case.rowdot:
        f.update(rowdot_with=next(px), rowdot_out=next(px), rowdot_T=case.rowdot)
    if case.dtype_ab == "fp8":
        f.update(alpha_a_dev=next(px), alpha_b_dev=next(px))
    if case.dtype_ab == "mx":
        f.update(mx_a=next(px), mx_b=next(px))
    if case.mx_out:
        f.update(mx_out=next(px), mx_out_scales=next(px))
    if case.split_k > 1 and not case.atomic:
        f["workspace"] = next(px)
        if case.via == "linear_wgrad":
            f["a_colsum"] = next(px)                         # ops.linear_wgrad: the fused bias gradient
    return f
