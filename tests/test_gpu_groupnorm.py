"""use_group_norm=True on the GPU: the GroupNorm(1, C) conv-module kernels against an fp64 CPU autograd reference,
the encoder against oracle.conformer.ConformerRef(use_group_norm=True), eval == train, batch independence, the
compiled-op route and HIP-graph capture.

Tolerances are the project's own: the kernel bounds of test_gpu_kernels.test_bn_folded_dwconv_bwd (the derived
bounds of tests/convmod_ref.py as relative L2, capped by 2e-2 bf16 / 1e-4 fp32; folded vs unfused 1e-5) and TOL /
ROWTOL of test_gpu_conformer."""
import pytest
import torch

import nn_conformer_for_speech_recognition_amd  # noqa: F401
from nn_conformer_for_speech_recognition_amd import _lib, ops
from nn_conformer_for_speech_recognition_amd.conformer import Conformer
from oracle import conformer as oc
from tests import convmod_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf, f32 = torch.bfloat16, torch.float32


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


rel_err = _rel

TOL = {f32: (1e-4, 1e-3), bf: (3e-2, 5e-2)}
ROWTOL = {f32: 1e-3, bf: 8e-2}


def row_max_err(y, yr, lens):
    y = torch.as_tensor(y).double().cpu()
    yr = torch.as_tensor(yr).double().cpu()
    worst = 0.0
    for b, n in enumerate(lens):
        d = (y[b, :n] - yr[b, :n]).abs().amax(-1) / yr[b, :n].abs().amax(-1).clamp_min(1e-30)
        worst = max(worst, d.max().item())
    return worst


# ----------------------------------------------------------------------------- 1. kernels
KCASES = [
    (2, 37, 64, 31, bf),       # one tile, T below 64
    (3, 100, 96, 3, f32),      # C not a multiple of 64, two time tiles
    (1, 129, 200, 33, bf),     # a one-frame last tile, C a multiple of 8 but not of 64
    (2, 50, 66, 31, bf),       # C not a multiple of 4: the scalar depthwise kernels and the scalar apply
    (2, 64, 512, 15, bf),      # L-width, vector paths
    (3, 7, 64, 31, f32),       # T shorter than the halo
    (2, 70, 72, 9, f32),       # no compiled K: the unfused fallback
]


@pytest.mark.parametrize("B,T,C,K,dt", KCASES)
def test_gn_convmod_kernels(B, T, C, K, dt):
    """cfm_gn_silu_fwd, cfm_gn_silu_bwd_sums + cfm_glu_dwconv_bwd_gn and the unfused cfm_gn_silu_bwd +
    cfm_glu_dwconv_bwd against a torch fp64 autograd reference of GLU -> depthwise conv -> F.group_norm(y, 1) ->
    SiLU.  Sample b's rows are scaled by 1 + b and its GLU inputs shifted by 0.5 b, so every sample has its own
    mean and variance: a statistic or coefficient indexed by the wrong sample fails.  The depthwise bias gradient is
    not zero here (GroupNorm does not cancel a per-channel bias) and is checked like the others."""
    g = torch.Generator().manual_seed(B * 1000 + T + C + K)
    a = torch.randn(B * T, 2 * C, generator=g)
    sample = torch.arange(B).repeat_interleave(T).float()[:, None]
    a = a * (1 + sample)
    a[:, :C] += 0.5 * sample
    w = torch.randn(C, K, generator=g) * 0.3
    bias = torch.randn(C, generator=g) * 0.1
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    dz = torch.randn(B * T, C, generator=g)
    # the reference sees what the kernels see: a and dz rounded to the dtype they are stored in
    a, dz = a.to(dt).float(), dz.to(dt).float()

    # reference (fp64, CPU autograd)
    ad = a.double().requires_grad_()
    wd, bd = w.double().requires_grad_(), bias.double().requires_grad_()
    gd, btd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    u = torch.nn.functional.glu(ad.view(B, T, 2 * C), dim=-1).transpose(1, 2)
    y = torch.nn.functional.conv1d(u, wd.view(C, 1, K), bd, padding=(K - 1) // 2, groups=C)
    z = torch.nn.functional.silu(torch.nn.functional.group_norm(y, 1, gd, btd, 1e-5))
    zr = z.transpose(1, 2).reshape(B * T, C)
    (zr * dz.double()).sum().backward()
    yd = y.detach()
    mu_ref = yd.mean(dim=(1, 2))
    rstd_ref = 1.0 / torch.sqrt(yd.var(dim=(1, 2), unbiased=False) + 1e-5)

    ad_, wd_, bd_ = a.to(DEV, dt), w.to(DEV), bias.to(DEV)
    gam, bet = gamma.to(DEV), beta.to(DEV)
    ws = ops.convmod_ws(B, T, C, K, DEV)
    yv = ops.glu_dwconv_fwd(ad_, wd_, bd_, B, T, C, K, ws)
    zv, mean, rstd = ops.gn_silu_fwd(yv, gam, bet, 1e-5, B, T, C, ws, dt)
    dzd = dz.to(DEV, dt)
    fold = ops.dwconv_bwd_folds(K)
    if fold:
        da, dw, db, dg, dbt = ops.gn_silu_glu_dwconv_bwd(dzd, yv, gam, bet, mean, rstd, ad_, wd_, B, T, C, K, ws, dt)
    dy, dg2, dbt2 = ops.gn_silu_bwd(dzd, yv, gam, bet, mean, rstd, B, T, ws)
    da2, dw2, db2 = ops.glu_dwconv_bwd(dy, ad_, wd_, B, T, C, K, ws, dt)
    torch.cuda.synchronize()
    if not fold:
        da, dw, db, dg, dbt = da2, dw2, db2, dg2, dbt2
    tol = 2e-2 if dt == bf else 1e-4
    # absolute, in units of the sample's standard deviation (a mean may be near zero); rstd relative
    stat = {"mean": ((mean.double().cpu() - mu_ref) * rstd_ref).abs().max().item(), "rstd": _rel(rstd, rstd_ref)}
    errs = {"z": _rel(zv.float(), zr.detach().to(dt).float() if dt == bf else zr.detach()),
            "da": _rel(da.float(), ad.grad), "dw": _rel(dw, wd.grad), "db": _rel(db, bd.grad),
            "dgamma": _rel(dg, gd.grad), "dbeta": _rel(dbt, btd.grad)}
    print("gn kernels", (B, T, C, K, dt), {k: f"{v:.2e}" for k, v in {**stat, **errs}.items()})
    assert mean.shape == (B,) and rstd.shape == (B,) and zv.dtype == dt
    # The fp32-side results against the element-wise bounds of tests/convmod_ref.py as relative L2,
    # ||(n + 8) 2^-24 S|| / ||ref|| with n the rows reduced plus what the stages before add end to end
    # (convmod_ref.upstream_ops); never looser than the earlier tol.  The reference is fed the rounded a and dz.
    M, u = B * T, R.U24
    yr, Sy = R.glu_dwconv_fwd(a, w, bias, B, T, C, K)
    st = R.gn_stats(yr, B, T, C, 1e-5)
    stage = (dz, yr, st.mean, st.invstd, gamma, beta)
    dbr, dgr, coef, Sb, Sg, _ = R.gn_bwd_sums(*stage, B, T)
    dyr, Sdy = R.gn_bwd_dy(*stage, coef, T)
    dar, dwr, dbr2, S_da, S_dw, S_db = R.glu_dwconv_bwd(dyr, a, w, B, T, C, K, Sdy)
    up = R.upstream_ops(K, yr, Sy)
    bound = {"z": tol, "da": R.rel_l2_bound(K + up, S_da, dar, dt == bf), "dw": R.rel_l2_bound(M + up, S_dw, dwr),
             "db": R.rel_l2_bound(M + up, S_db, dbr2), "dgamma": R.rel_l2_bound(M + up, Sg, dgr),
             "dbeta": R.rel_l2_bound(M + up, Sb, dbr)}
    # the statistics: the one-pass sums' STAT_ADDS 2^-24 (sqrt(E[y^2]) for the mean, E[y^2] for the variance) plus
    # the forward's own (K + 8) 2^-24 S_y carried into them; rstd relative: half the variance's, + its fp32 store
    S3 = Sy.reshape(B, -1)
    bmean = (R.STAT_ADDS * u * st.ey2.sqrt() + (K + 8) * u * S3.mean(1)) * st.invstd
    dvar = R.STAT_ADDS * u * st.ey2 + 2 * st.var.sqrt() * (K + 8) * u * (S3 ** 2).mean(1).sqrt()
    sbound = {"mean": bmean.max().item(), "rstd": (0.5 * dvar / (st.var + 1e-5) + u).max().item()}
    print("  bounds", {k: f"{min(v, tol):.2e}" for k, v in {**sbound, **bound}.items()})
    # the statistics are fp32 from fp32 y (bf16 enters only through a): a wrong-sample index is off by O(1)
    for k, v in stat.items():
        assert v < min(sbound[k], tol), (k, v, sbound[k])
    for k, v in errs.items():
        assert v < min(bound[k], tol), (k, v, bound[k])
    if fold:    # same formula and the same parameter-gradient sums as the unfused pair
        pair = {"da": _rel(da.float(), da2.float()), "dw": _rel(dw, dw2), "db": _rel(db, db2)}
        print("  folded vs unfused", {k: f"{v:.2e}" for k, v in pair.items()})
        assert pair["da"] < 1e-5
        assert pair["dw"] < 1e-5 and pair["db"] < 1e-5
        assert torch.equal(dg, dg2) and torch.equal(dbt, dbt2)


# ----------------------------------------------------------------------------- 2. encoder vs the oracle
CASES = [
    # d, H, ffn, K, layers, B, T, lens, conv_first, pos   (ragged lengths: the statistics include padded frames)
    (256, 4, 1024, 31, 2, 4, 200, [200, 150, 77, 1], False, "none"),
    (144, 4, 576, 31, 2, 3, 130, [130, 129, 64], True, "none"),
    (128, 2, 256, 15, 1, 2, 96, [96, 50], False, "rel"),
    (512, 8, 2048, 31, 1, 2, 373, [373, 300], False, "none"),
]
_ORACLE = {}


def _oracle_run(case):
    """The CPU oracle's forward + backward of one case, computed once and shared by both compute dtypes."""
    if case not in _ORACLE:
        d, H, ffn, K, L, B, T, lens, conv_first, pos = CASES[case]
        torch.manual_seed(7)
        ref = oc.ConformerRef(d, H, ffn, L, K, 0.0, use_group_norm=True, convolution_first=conv_first,
                              pos_enc=pos).train()
        with torch.no_grad():
            for n, prm in ref.named_parameters():
                if n.endswith("bias"):
                    prm.normal_(0, 0.05)
                if n.endswith("conv_module.sequential.3.weight"):
                    prm.uniform_(0.5, 1.5)
        x = torch.randn(B, T, d)
        xr = x.clone().requires_grad_()
        yr, _ = ref(xr, torch.tensor(lens))
        gy = torch.randn_like(yr)
        yr.backward(gy)
        _ORACLE[case] = (ref.state_dict(), x, gy, yr.detach(), xr.grad,
                         {n: p.grad for n, p in ref.named_parameters()})
    return _ORACLE[case]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("cd", [f32, bf])
def test_gn_encoder_vs_oracle(case, cd):
    d, H, ffn, K, L, B, T, lens, conv_first, pos = CASES[case]
    sd, x, gy, yr, gxr, gpr = _oracle_run(case)
    m = Conformer(d, H, ffn, L, K, 0.0, use_group_norm=True, convolution_first=conv_first, pos_enc=pos,
                  compute_dtype=cd)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    assert len(list(m.buffers())) == 0
    xd = x.to(DEV).requires_grad_()
    y, _ = m(xd, torch.tensor(lens).to(DEV))
    y.backward(gy.to(DEV))
    tol_y, tol_g = TOL[cd]
    errs = {"y": rel_err(y.detach(), yr), "rows": row_max_err(y.detach(), yr, lens), "dx": rel_err(xd.grad, gxr)}
    for n, prm in m.named_parameters():
        assert prm.grad is not None, n
        errs[n] = rel_err(prm.grad, gpr[n])
    worst = max((v, k) for k, v in errs.items() if k not in ("y", "rows", "dx"))
    print("gn encoder", case, cd, {k: f"{errs[k]:.2e}" for k in ("y", "rows", "dx")}, "worst grad", worst)
    assert errs["y"] < tol_y
    assert errs["rows"] < ROWTOL[cd]
    assert errs["dx"] < tol_g
    for n, _ in m.named_parameters():
        assert errs[n] < tol_g * (3 if "pos_bias" in n else 1), (n, errs[n])
    assert len(list(m.buffers())) == 0


# ----------------------------------------------------------------------------- 3. eval
def test_gn_eval_matches_oracle_and_train():
    """No train / eval difference: eval equals the oracle's eval, and a train-mode forward with dropout 0 equals the
    eval forward of the same module bit for bit."""
    torch.manual_seed(3)
    d, H, ffn, K = 64, 2, 128, 7
    ref = oc.ConformerRef(d, H, ffn, 1, K, 0.1, use_group_norm=True)
    with torch.no_grad():
        gn = ref.conformer_layers[0].conv_module.sequential[3]
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_(0, 0.1)
    ref.eval()
    m = Conformer(d, H, ffn, 1, K, 0.1, use_group_norm=True, compute_dtype=f32)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    x = torch.randn(2, 40, d)
    ln = torch.tensor([40, 33])
    with torch.no_grad():
        yr, _ = ref(x, ln)
        y, _ = m(x.to(DEV), ln.to(DEV))
        assert rel_err(y, yr) < 1e-4
        m.train()
        for ly in m.conformer_layers:
            ly.dropout = 0.0
        yt, _ = m(x.to(DEV), ln.to(DEV))
    assert torch.equal(yt, y)
    assert len(list(m.buffers())) == 0


# ----------------------------------------------------------------------------- 4. batch independence
def test_gn_batch_independence():
    """The property data parallelism relies on: with per-utterance statistics, sample b of a batched run equals the
    run of that sample alone, and the batched parameter gradients are the sum of the single-sample gradients.
    (With use_group_norm=False the same assertions fail: BatchNorm's statistics are over the whole batch.)"""
    torch.manual_seed(5)
    d, H, ffn, K, L, B, T = 64, 2, 128, 7, 2, 3, 50
    m = Conformer(d, H, ffn, L, K, 0.0, use_group_norm=True, compute_dtype=f32).to(DEV).train()
    with torch.no_grad():
        for n, prm in m.named_parameters():
            if n.endswith("bias"):
                prm.normal_(0, 0.05)
    x = torch.randn(B, T, d, device=DEV) * (1 + torch.arange(B, device=DEV).float())[:, None, None]
    gy = torch.randn(B, T, d, device=DEV)
    ln = torch.full((B,), T, device=DEV)
    y, _ = m(x, ln)
    y.backward(gy)
    batched = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    for b in range(B):
        yb, _ = m(x[b:b + 1], ln[b:b + 1])
        assert rel_err(yb[0], y[b].detach()) < 1e-4, b
        yb.backward(gy[b:b + 1])          # .grad accumulates the three single-sample gradients
    for n, p in m.named_parameters():
        assert rel_err(batched[n], p.grad) < 1e-3, n


# ----------------------------------------------------------------------------- 5. compiled-op route
def _r(*shape, dtype=f32, seed=0, scale=1.0, grad=False):
    t = (torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * scale).to(dtype)
    return t.requires_grad_(grad)


def test_gn_opcheck():
    c = torch.ops.cfm
    args = (_r(2 * 40, 2 * 64, dtype=bf, grad=True), _r(64, 31, seed=1, scale=0.2, grad=True),
            _r(64, seed=2, grad=True), (1 + 0.1 * _r(64, seed=3)).requires_grad_(), _r(64, seed=4, grad=True),
            1e-5, 2, bf)
    torch.library.opcheck(c.conv_glu_dwconv_gn_silu.default, args)
    a, w, b_dw, gamma, beta = (t.detach() for t in args[:5])
    z, y, mean, rstd = c.conv_glu_dwconv_gn_silu(a, w, b_dw, gamma, beta, 1e-5, 2, bf)
    torch.library.opcheck(c.conv_glu_dwconv_gn_silu_bwd.default,
                          (_r(2 * 40, 64, dtype=bf, seed=5), a, y, w, gamma, beta, mean, rstd, 2))


def _gn_models(dropout, conv_first=False):
    torch.manual_seed(0)
    m = Conformer(144, 4, 576, 2, 31, dropout=dropout, use_group_norm=True, convolution_first=conv_first).to(DEV)
    with torch.no_grad():
        for ly in m.conformer_layers:
            gn = ly.conv_module.sequential[3]
            gn.weight.uniform_(0.5, 1.5)
            gn.bias.normal_(0, 0.1)
    m2 = Conformer(144, 4, 576, 2, 31, dropout=dropout, use_group_norm=True, convolution_first=conv_first).to(DEV)
    m2.load_state_dict(m.state_dict())
    return m, m2


def test_gn_compiled_encoder_eval_matches_fused():
    m, m2 = _gn_models(0.1, conv_first=True)
    m.eval()
    m2.eval()
    x = _r(3, 97, 144, seed=21)
    lens = torch.tensor([97, 60, 33], device=DEV)
    with torch.no_grad():
        ref, _ = m(x, lens)
        torch._dynamo.reset()
        y, _ = torch.compile(m2, fullgraph=True, backend="aot_eager")(x, lens)
    torch.cuda.synchronize()
    assert _rel(y, ref) < 1e-5


def test_gn_compiled_encoder_train_matches_fused():
    """library.layer_forward on GroupNorm layers (torch.compile, fullgraph, AOTAutograd over the registered backward
    op) vs the fused layer node with the same dropout seeds: output, input gradient, every parameter gradient."""
    m, m2 = _gn_models(0.1)
    m.train()
    m2.train()
    B, T = 2, 80
    x = _r(B * T, 144, seed=31)
    lens = torch.tensor([80, 51], device=DEV, dtype=torch.int32)
    g = _r(B * T, 144, seed=32)
    x1 = x.clone().requires_grad_()
    y1 = m.forward_tokens(x1, lens, B, T, seed=777)
    (y1 * g).sum().backward()
    x2 = x.clone().requires_grad_()
    torch._dynamo.reset()
    y2 = torch.compile(m2.forward_tokens, fullgraph=True, backend="aot_eager")(x2, lens, B, T, 777)
    (y2 * g).sum().backward()
    torch.cuda.synchronize()
    assert _rel(y2, y1) < 1e-5
    assert _rel(x2.grad, x1.grad) < 2e-2
    p1, p2 = dict(m.named_parameters()), dict(m2.named_parameters())
    for n in p1:
        assert _rel(p2[n].grad, p1[n].grad) < 2e-2, n
    assert len(list(m2.buffers())) == 0


# ----------------------------------------------------------------------------- 6. HIP-graph capture
def test_gn_graph_replay_matches_eager():
    """One forward + backward of a 2-layer GroupNorm encoder captured into a HIP graph: each replay equals the eager
    step at the same dropout-counter value bit for bit."""
    torch.manual_seed(0)
    B, T, d = 3, 40, 64
    model = Conformer(d, 2, 128, 2, 7, dropout=0.1, use_group_norm=True).to(DEV).train()
    x = torch.randn(B * T, d, device=DEV)
    gy = torch.randn(B * T, d, device=DEV)
    lens = torch.tensor([T, T - 7, 25], dtype=torch.int32, device=DEV)
    params = list(model.parameters())
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    _lib.call("cfm_rng_bind", _lib.ptr(ctr))
    try:
        def step():
            ctr.add_(1)
            y = model.forward_tokens(x, lens, B, T, seed=5)
            y.backward(gy)
            return y.detach()

        def grads():
            return torch.cat([p.grad.reshape(-1) for p in params]).clone()

        eager = []
        for _ in range(2):
            for p in params:
                p.grad = None
            eager.append((step().clone(), grads()))
        assert not torch.equal(eager[0][0], eager[1][0])       # counter 1 vs 2: different masks

        ctr.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up outside the capture
            for p in params:
                p.grad = None
            step()
        torch.cuda.current_stream().wait_stream(side)
        for p in params:
            p.grad = None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static = step()
        for i, (want_y, want_grad) in enumerate(eager):
            ctr.fill_(i)                                       # the captured add_(1) makes it i + 1
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(static, want_y)
            assert torch.equal(grads(), want_grad)
    finally:
        _lib.call("cfm_rng_bind", None)
