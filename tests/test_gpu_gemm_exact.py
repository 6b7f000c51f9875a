"""Every GEMM kernel variant against the exact answer, element by element, inside guard bands (tests/gemm_exact.py).

Integer operands make the int64 product the only right answer: an fp32 C must equal it, a bf16 C its round-to-nearest-even
cast (the kernels convert with the compiler's (bf16) cast) -- no tolerance, so one wrong row, one wrong 8-column chunk or
an off-by-one at a tile edge fails and is named.  Each case also asserts the variant and the epilogue kind it launched,
that no guard, padding or inter-batch position of an output changed (raw bits), and that the NaN in every guard and
padding position of its inputs reached no stored element.

Not exact, by construction: SiLU outputs (the stored pre-activation is exact and asserted so; silu(pre) is held to
fp64 silu(pre) within RTOL[dtype] + 2e-6 relative, atol 0 -- the per-element tolerance of test_gpu_dropout_masks.py) and
act_grad with pre = 0 (acc / 2, same tolerance).  Dropout stays off: its masks are read back exactly there.

The real-valued cases (randn operands, fp64 reference) hold every element to the forward bound of a length-K fp32 dot
product in any order, |C - ref| <= (K + 2) 2^-23 (|A| |B|^T) (+ 2^-8 |ref| for a bf16 C): u = 2^-23 covers truncating
accumulation, the + 2 alpha and the bias add -- integers cannot show a precision loss that stays exact on integers."""
import zlib

import numpy as np
import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ops
from tests import gemm_exact as ge
from tests.gemm_exact import BF, F32, F8, U8, assert_untouched, guarded, int_matmul, int_operand

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = {F32: 2.0 ** -23, BF: 2.0 ** -8}      # as test_gpu_dropout_masks.RTOL
SILU_EXTRA = 2e-6
_VNAME = {v: k for k, v in vars(_lib).items() if k.startswith("GEMM_V_")}
_ENAME = {v: k for k, v in vars(_lib).items() if k.startswith("GEMM_EPI_")}


@pytest.fixture
def gemm_mode():
    yield from ge.gemm_mode_fixture()


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _equal(got, want, what):
    """every element equal (values; NaN anywhere fails), the first offenders named"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.double(), want.double()
    assert not torch.isnan(g).any(), (what, "NaN stored (an input guard or padding value was read): first at",
                                      torch.isnan(g).nonzero()[:4].tolist(), int(torch.isnan(g).sum()), "elements")
    if not torch.equal(g, w):
        first, n = ge.first_mismatches(g, w)
        raise AssertionError(f"{what}: {n} of {g.numel()} elements differ; (index, got, want): {first}")


def _close(got, ref, rtol, what):
    """|got - ref| <= rtol |ref| for every element (atol 0)"""
    g, r = got.cpu().double(), ref.double()
    assert not torch.isnan(g).any(), (what, "NaN stored", torch.isnan(g).nonzero()[:4].tolist())
    bad = (g - r).abs() > rtol * r.abs()
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements off by more than {rtol:.3g} relative; "
                             f"first {i}: got {g[i].item()!r}, reference {r[i].item()!r}")


def _silu64(x):
    return x / (1.0 + torch.exp(-x))


def _operand(case, which, gen, real):
    """-> (logical (batch, rows_mn, K) CPU tensor in the operand's host dtype, Guarded device buffer holding it in the
    case's layout).  B is shared by the batches (stride_b 0)."""
    a = which == "a"
    mn, kmajor, ld = (case.M, case.a_kmajor, case.lda) if a else (case.N, case.b_kmajor, case.ldb)
    batch = case.batch if a else 1
    dt = ge.DTYPES.get(case.dtype_ab, BF)          # fp8 / mx: quantised on the device from bf16
    K = case.K
    fan = 256 if case.rowdot else 2                # rowdot: 64 columns x |with| <= 4; else alpha / out_scale <= 2
    if a and case.overlap:
        flat = int_operand(((mn - 1) * ld + K,), dt, gen, case.lo, case.hi, k=K, fan_in=fan)
        g = guarded(mn, K, ld, dt, "nan", device=DEV)
        g.flat.copy_(flat)
        return flat.unfold(0, K, ld).unsqueeze(0), g
    if real:
        x = torch.randn(batch, mn, K, generator=gen).to(dt)
    else:
        x = int_operand((batch, mn, K), dt, gen, case.lo, case.hi, k=K, fan_in=fan)
    stored = x if kmajor else x.transpose(1, 2)
    rows, cols = stored.shape[1:]
    return x, guarded(rows, cols, ld, dt, "nan", batch=batch, device=DEV).set(stored)


def _quantise(case, x, ld, what):
    """the integer operand x (1, rows, K) quantised on the device, the quantisation asserted to round-trip exactly
    -> (Guarded e4m3 operand, scale argument: the per-tensor device scalar or the Guarded e8m0 block-scale rows)"""
    rows, K = x.shape[1:]
    xd = x[0].to(DEV).contiguous()
    if case.dtype_ab == "fp8":
        q, s = ops.quant_fp8(xd)
        back = torch.empty(rows, K, device=DEV)
        _lib.call("cfm_dequant_fp8", _lib.ptr(q), rows * K, _lib.ptr(s), _lib.ptr(back), _lib.stream())
        scale = s
    else:
        q, s = ops.quant_mx(xd)
        back = ops.dequant_mx(q, s)
        scale = guarded(rows, K // 32, K // 32, U8, "nan", device=DEV).set(s)
    _equal(back, x[0].float(), (case.id, what, "quantisation round trip"))
    return guarded(rows, K, ld, F8, "nan", device=DEV).set(q), scale


def _launch(case, gemm_mode, real=False):
    """builds the case's operands in guarded buffers, launches it under its mode -> everything the checks need"""
    M, N, K, Z = case.M, case.N, case.K, case.batch
    cdt = ge.DTYPES[case.dtype_c]
    gen = _gen(case.id)
    A, gA = _operand(case, "a", gen, real)
    B, gB = _operand(case, "b", gen, real)
    r = dict(A=A, B=B[0], outs=[])
    kw = dict(a_kmajor=case.a_kmajor, b_kmajor=case.b_kmajor, lda=case.lda, ldb=case.ldb, ldc=case.ldc, alpha=case.alpha,
              out_scale=case.out_scale, split_k=case.split_k, allow_overlap=case.overlap)
    a_arg, b_arg = gA.view, gB.view
    if case.dtype_ab in ("fp8", "mx"):
        gA, sa = _quantise(case, A, case.lda, "A")
        gB, sb = _quantise(case, B, case.ldb, "B")
        a_arg, b_arg = gA.view, gB.view
        kw.update(dict(alpha_a=sa, alpha_b=sb) if case.dtype_ab == "fp8" else dict(mx_a=sa.view, mx_b=sb.view))
    # outputs: the sentinel in guards and padding, NaN in the logical region (an element never stored then fails)
    gC = guarded(M, N, case.ldc, cdt, "sentinel", batch=Z, device=DEV).poison()
    r["C"] = gC
    r["outs"].append(("C", gC))
    if Z > 1:
        kw.update(batch=Z, stride_a=gA.stride, stride_b=0, stride_c=gC.stride)
    if case.bias:
        r["bias"] = (torch.randn(N, generator=gen) if real else int_operand((N,), F32, gen, case.lo, case.hi, k=1))
        kw["bias"] = guarded(1, N, N, F32, "nan", device=DEV).set(r["bias"][None]).view[0, 0]
    if case.pre:
        pdt = ge.DTYPES[case.pre]                   # indexed like C: ldc and stride_c
        gP = guarded(M, N, case.ldc, pdt, "nan" if case.act_grad else "sentinel", batch=Z, device=DEV)
        if case.act_grad:
            gP.view.zero_()
            kw["act_grad"] = True
        else:
            gP.poison()
            r["pre"] = gP
            r["outs"].append(("pre", gP))
        kw["pre"] = gP.view
    if case.act:
        kw["act"] = ops.ACT_SILU
    if case.residual:
        rdt = ge.DTYPES[case.residual]
        ldr = case.ldc if Z > 1 else N + 16          # batches follow stride_c
        r["residual"] = int_operand((Z, M, N), rdt, gen, case.lo, case.hi, k=1)
        gR = guarded(M, N, ldr, rdt, "nan", batch=Z, device=DEV).set(r["residual"])
        assert Z == 1 or gR.stride == gC.stride
        kw.update(residual=gR.view, ldr=ldr)
    if case.rowdot:
        r["with"] = int_operand((M, N), BF, gen, case.lo, case.hi, k=1)
        gW = guarded(M, N, case.ldc, BF, "nan", device=DEV).set(r["with"])
        r["D"] = guarded(1, M * N // 64, M * N // 64, F32, "sentinel", device=DEV).poison()
        r["outs"].append(("rowdot", r["D"]))
        kw["rowdot"] = (gW.view, r["D"].view, case.rowdot)
    if case.mx_out:
        r["y8"] = guarded(M, N, N, F8, "sentinel", device=DEV).poison()
        r["s8"] = guarded(M, N // 32, N // 32, U8, "sentinel", device=DEV).poison()
        r["outs"] += [("mx_out", r["y8"]), ("mx_out scales", r["s8"])]
        kw["mx_out"] = (r["y8"].view, r["s8"].view)
    if case.atomic:
        gC.view.zero_()
    elif case.split_k > 1 and case.via == "gemm":      # slabs: unwritten ones would show as NaN
        kw["workspace"] = torch.full((case.split_k * Z * M * N,), float("nan"), device=DEV)
    gemm_mode(ge.mode_value(case.mode))
    with ge.planned() as seen:
        if case.via == "linear_wgrad":
            r["db"] = guarded(1, M, M, F32, "sentinel", device=DEV).poison()
            r["outs"].append(("bias_out", r["db"]))
            ops.linear_wgrad(gA.view[0], gB.view[0], out=gC.view[0], split_k=case.split_k, bias_out=r["db"].view[0, 0])
        else:
            ops.gemm(a_arg, b_arg, gC.view, M, N, K, **kw)
    torch.cuda.synchronize()
    assert len(seen) == 1, seen
    assert seen[0] == (case.variant, case.epilogue), (
        case.id, "launched", _VNAME[seen[0][0]], _ENAME[seen[0][1]], "the row names", _VNAME[case.variant],
        _ENAME[case.epilogue])
    for name, g in r["outs"]:
        assert_untouched(g, f"{case.id} {name}")
    return r


@pytest.mark.parametrize("case", ge.INT_CASES, ids=[c.id for c in ge.INT_CASES])
def test_gemm_exact(gemm_mode, case):
    r = _launch(case, gemm_mode)
    cdt = ge.DTYPES[case.dtype_c]
    v = case.alpha * int_matmul(r["A"], r["B"]).double()          # (batch, M, N), exact
    if case.bias:
        v = v + r["bias"].double()
    got = r["C"].view
    if case.via == "linear_wgrad":
        _equal(r["db"].view[0, 0], r["A"][0].long().sum(-1).float(), (case.id, "bias_out = column sums of dy"))
    if case.act_grad:                                              # pre = 0: silu'(0) = 1/2
        _close(got, 0.5 * v, RTOL[cdt] + SILU_EXTRA, (case.id, "act_grad"))
        return
    if case.act:
        # premise of the relative comparison: silu(pre) is a normal number in fp32 / bf16 (x e^x underflows below ~ -87)
        assert float(v.abs().max()) <= 80, (case.id, "test premise: |pre| <= 80", float(v.abs().max()))
        _equal(r["pre"].view, v.float().to(r["pre"].dtype), (case.id, "stored pre-activation"))
        ref = case.out_scale * _silu64(v)
        _close(got, ref, RTOL[cdt] + SILU_EXTRA, (case.id, "silu output"))
        if case.mx_out:                                            # exactly quant_mx of the bf16 C, element by element
            q, s = ops.quant_mx(got[0].contiguous())
            _equal(r["s8"].bits[0], s, (case.id, "mx_out block scales"))
            _equal(r["y8"].bits[0], q.view(torch.uint8), (case.id, "mx_out e4m3 bytes"))
        return
    v = v * case.out_scale
    if case.residual:
        v = v + r["residual"].double()
    assert float(v.abs().max()) < ge.EXACT_LIMIT / 2
    want = v.float().to(cdt)
    _equal(got, want, (case.id, "C"))
    if case.rowdot:       # D[b][g][t] = sum over the 64 columns of group g of bf16(C)[b T + t][n] * with[b T + t][n]
        T = case.rowdot
        p = (want[0].double() * r["with"].double()).reshape(case.M // T, T, case.N // 64, 64).sum(-1)
        _equal(r["D"].view[0, 0], p.permute(0, 2, 1).reshape(-1).float(), (case.id, "rowdot"))


@pytest.mark.parametrize("case", ge.REAL_CASES, ids=[c.id for c in ge.REAL_CASES])
def test_gemm_real_valued_forward_bound(gemm_mode, case):
    """randn operands (rounded to the operand dtype), fp64 reference: every element within (K + 2) 2^-23 (|A| |B|^T)
    (+ 2^-8 |ref| for bf16 C) -- derived, not tuned (module docstring)."""
    r = _launch(case, gemm_mode, real=True)
    A, B = r["A"].double(), r["B"].double()
    ref = A @ B.T + r["bias"].double()
    bound = (case.K + 2) * 2.0 ** -23 * (A.abs() @ B.abs().T)
    if case.dtype_c == "bf16":
        bound = bound + 2.0 ** -8 * ref.abs()
    got = r["C"].view.cpu().double()
    assert not torch.isnan(got).any(), (case.id, "NaN stored", torch.isnan(got).nonzero()[:4].tolist())
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    print(f"{case.id}: max |C - ref| / bound = {ratio:.4f}")
    bad = err > bound
    assert not bad.any(), (case.id, int(bad.sum()), "elements past the bound; first", bad.nonzero()[:4].tolist(),
                           "worst error / bound", ratio)


# ------------------------------------------------------------------------------------------ grouped weight gradients
WGROUP_SHAPES = [(136, 72), (264, 136), (512, 520)]      # (N, K) of each dW: ragged against the 256 x 256 tile


@pytest.mark.parametrize("plan", [True, False], ids=["planned", "unplanned"])
@pytest.mark.parametrize("M", [37, 1000])
def test_wgrad_group_exact(monkeypatch, M, plan):
    """cfm_wgrad_group over one group of three dW = dy^T x (+ db = column sums of dy), token counts that are no
    multiple of the 32-deep K step, with the XCD-aware plan (split ragged rounds, slab reduction) and without."""
    monkeypatch.setattr(ops, "WGRAD_PLAN", plan)
    gen = _gen(f"wgroup{M}")
    grp = ops.WgradGroup()
    held = []
    for N, K in WGROUP_SHAPES:
        dy = int_operand((M, N), BF, gen, k=M)
        x = int_operand((M, K), BF, gen, k=M)
        gdy = guarded(M, N, N, BF, "nan", device=DEV).set(dy)
        gx = guarded(M, K, K, BF, "nan", device=DEV).set(x)
        gdw = guarded(N, K, K, F32, "sentinel", device=DEV).poison()
        gdb = guarded(1, N, N, F32, "sentinel", device=DEV).poison()
        assert ops.wgrad_group_ok(gdy.view[0], gx.view[0])
        grp.add(gdy.view[0], gx.view[0], dest=(gdw.view[0], gdb.view[0, 0]))
        held.append((dy, x, gdy, gx, gdw, gdb))
    grp.flush()
    torch.cuda.synchronize()
    for (N, K), (dy, x, _, _, gdw, gdb) in zip(WGROUP_SHAPES, held):
        assert_untouched(gdw, f"dW {N}x{K}")
        assert_untouched(gdb, f"db {N}")
        _equal(gdw.view[0], (dy.long().T @ x.long()).float(), ("dW", M, N, K, plan))
        _equal(gdb.view[0, 0], dy.long().sum(0).float(), ("db", M, N, plan))


# ------------------------------------------------------------------------------------------ convolutions
CONV_SHAPES = [(1, 9, 11, 64, 32), (2, 10, 8, 128, 64)]     # (B, F1, T1, C1, C2)
CONV_MODES = [("default", _lib.GEMM_MODE_DEFAULT), ("staged", _lib.GEMM_MODE_STAGED256)]


def _gin(t, dtype=BF):
    """an input tensor in a NaN-guarded buffer (contiguous: the guards are before and after it)"""
    n = t.numel()
    g = guarded(1, n, n, dtype, "nan", device=DEV).set(t.reshape(1, n).to(dtype))
    return g.view[0, 0]


def _gout(shape, dtype):
    rows, cols = int(np.prod(shape[:-1])), shape[-1]
    return guarded(rows, cols, cols, dtype, "sentinel", device=DEV).poison()


def _conv2_data(B, F1, T1, C1, C2):
    gen = _gen(f"conv2-{B}-{F1}-{T1}-{C1}-{C2}")
    F2, T2 = (F1 - 3) // 2 + 1, (T1 - 3) // 2 + 1
    W = torch.randint(-4, 5, (C2, C1, 3, 3), generator=gen)
    h1 = torch.randint(-4, 5, (B, F1, T1, C1), generator=gen)
    dh2 = torch.randint(-4, 5, (B, T2, F2, C2), generator=gen)
    b2 = torch.randint(-4, 5, (C2,), generator=gen)
    assert 16 * 9 * C1 < ge.EXACT_LIMIT and 16 * B * F2 * T2 < ge.EXACT_LIMIT
    return W, W.permute(0, 2, 3, 1).reshape(C2, 9 * C1).contiguous(), h1, dh2, b2, F2, T2


@pytest.mark.parametrize("mode", CONV_MODES, ids=[m[0] for m in CONV_MODES])
@pytest.mark.parametrize("B,F1,T1,C1,C2", CONV_SHAPES)
def test_conv2_exact(gemm_mode, mode, B, F1, T1, C1, C2):
    """conv2 forward (fp32 and bf16 h2), data gradient and weight gradient on integer data against int64 conv2d /
    conv_transpose2d, in the LDS-DMA (gathered operand) and the register-staged gather kernels; outputs in guards."""
    W, w2r, h1, dh2, b2, F2, T2 = _conv2_data(B, F1, T1, C1, C2)
    gemm_mode(mode[1])
    h1d, w2d, dh2d, b2d = _gin(h1), _gin(w2r), _gin(dh2), _gin(b2, F32)
    st = _lib.stream()
    fwd = torch.nn.functional.conv2d(h1.permute(0, 3, 1, 2), W, b2, stride=2).permute(0, 3, 2, 1)    # (B, T2, F2, C2)
    for dt in (F32, BF):
        g = _gout((B, T2, F2, C2), dt)
        _lib.call("cfm_conv2_fwd", _lib.ptr(h1d), _lib.ptr(w2d), _lib.ptr(b2d), _lib.ptr(g.view), _lib.dt(g.view),
                  _lib.BF16, B, F1, T1, C1, C2, st)
        torch.cuda.synchronize()
        assert_untouched(g, f"conv2_fwd {dt}")
        _equal(g.view.reshape(B, T2, F2, C2), fwd.float().to(dt), ("conv2_fwd", mode[0], dt))
    # data gradient: the transposed convolution
    dgrad = torch.nn.functional.conv_transpose2d(dh2.permute(0, 3, 2, 1), W, stride=2,
                                                 output_padding=(F1 - (2 * F2 + 1), T1 - (2 * T2 + 1))).permute(0, 2, 3, 1)
    g = _gout((B, F1, T1, C1), BF)
    ws = torch.full((_lib.size_call("cfm_conv2_bwd_data_ws_bytes", C1, C2) // 2,), float("nan"), device=DEV, dtype=BF)
    _lib.call("cfm_conv2_bwd_data_ws", _lib.ptr(dh2d), _lib.ptr(w2d), _lib.ptr(g.view), _lib.BF16, B, F1, T1, C1, C2,
              _lib.ptr(ws), st)
    torch.cuda.synchronize()
    assert_untouched(g, "conv2_bwd_data")
    _equal(g.view.reshape(B, F1, T1, C1), dgrad.float().to(BF), ("conv2_bwd_data", mode[0]))
    # weight gradient: dW[c2][kh][kw][c1] = sum over (b, f2, t2) of dh2[b, t2, f2, c2] h1[b, 2 f2 + kh, 2 t2 + kw, c1]
    wg = torch.empty(C2, 3, 3, C1, dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            win = h1[:, kh:kh + 2 * F2:2, kw:kw + 2 * T2:2, :]                       # (B, F2, T2, C1)
            wg[:, kh, kw, :] = torch.einsum("btfo,bftc->oc", dh2, win)
    nb = _lib.size_call("cfm_conv2_bwd_weight_ws_bytes", B, F1, T1, C1, C2)
    for slabs in ([False, True] if nb else [False]):
        g = _gout((C2, 9 * C1), F32)
        wsw = torch.full((nb // 4,), float("nan"), device=DEV) if slabs else None
        _lib.call("cfm_conv2_bwd_weight_ws", _lib.ptr(dh2d), _lib.ptr(h1d), _lib.ptr(g.view), _lib.BF16, B, F1, T1, C1,
                  C2, _lib.ptr(wsw), st)
        torch.cuda.synchronize()
        assert_untouched(g, "conv2_bwd_weight")
        _equal(g.view[0], wg.reshape(C2, 9 * C1).float(), ("conv2_bwd_weight", mode[0], "slabs" if slabs else "one slice"))


@pytest.mark.parametrize("B,F1,T1,C1", [(1, 9, 11, 64), (2, 10, 8, 128), (1, 9, 11, 512)])
def test_conv1_exact(B, F1, T1, C1):
    """conv1 (1 -> C1 channels, 7 x 7, stride 2) forward and weight / bias gradient on integer data against int64
    conv2d (C1 512: the matrix-core kernels); outputs in guards."""
    gen = _gen(f"conv1-{B}-{F1}-{T1}-{C1}")
    F, T = 2 * (F1 - 1) + 7, 2 * (T1 - 1) + 7
    x = torch.randint(-4, 5, (B, F, T), generator=gen)
    w = torch.randint(-4, 5, (C1, 49), generator=gen)
    b = torch.randint(-4, 5, (C1,), generator=gen)
    dh1 = torch.randint(-4, 5, (B, F1, T1, C1), generator=gen)
    xd, wd, bd, dhd = _gin(x, F32), _gin(w, F32), _gin(b, F32), _gin(dh1)
    st = _lib.stream()
    ref = torch.nn.functional.conv2d(x.unsqueeze(1), w.view(C1, 1, 7, 7), b, stride=2).permute(0, 2, 3, 1)
    for dt in (BF, F32):
        g = _gout((B, F1, T1, C1), dt)
        _lib.call("cfm_conv1_fwd", _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(g.view), _lib.dt(g.view), B, F, T,
                  C1, st)
        torch.cuda.synchronize()
        assert_untouched(g, f"conv1_fwd {dt}")
        _equal(g.view.reshape(B, F1, T1, C1), ref.float().to(dt), ("conv1_fwd", dt))
    # dw1[c][kh][kw] = sum over (b, f1, t1) of dh1[b, f1, t1, c] x[b, 2 f1 + kh, 2 t1 + kw];  db1 = sum dh1
    dw = torch.empty(C1, 7, 7, dtype=torch.int64)
    for kh in range(7):
        for kw in range(7):
            dw[:, kh, kw] = torch.einsum("bftc,bft->c", dh1, x[:, kh:kh + 2 * F1:2, kw:kw + 2 * T1:2])
    gw, gb = _gout((C1, 49), F32), _gout((1, C1), F32)
    ws = ops.workspace(_lib.size_call("cfm_conv1_bwd_ws_bytes", B, F, T, C1), DEV)
    _lib.call("cfm_conv1_bwd_weight", _lib.ptr(dhd), _lib.BF16, _lib.ptr(xd), _lib.ptr(gw.view), _lib.ptr(gb.view), B,
              F, T, C1, _lib.ptr(ws), st)
    torch.cuda.synchronize()
    assert_untouched(gw, "conv1 dw")
    assert_untouched(gb, "conv1 db")
    _equal(gw.view[0], dw.reshape(C1, 49).float(), "conv1_bwd_weight dw1")
    _equal(gb.view[0, 0], dh1.sum((0, 1, 2)).float(), "conv1_bwd_weight db1")
