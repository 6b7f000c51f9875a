"""Values and gradients with dropout ON against references that are not this library: torch autograd over the masks
of the numpy restatement (tests/dropout_hash.py).  The trained configuration (dropout 0.1) gets the footing the
dropout-free path has in test_attention_vs_torch / test_rel_attention_vs_torch / test_gemm_epilogues /
test_encoder_vs_oracle / test_fold_vs_fp64_composition:

* the attention core (every kernel family and backward variant) against the fp32 torch restatement with probs * keep;
* one residual FFN module at kernel level, called exactly as conformer._ffn_fwd / _ffn_bwd call the kernels, against
  an fp64 torch FFN under the two helper masks;
* the whole encoder against oracle.ConformerRef in fp64 under a mask provider built from the seed map RESTATED here
  (forward and backward seeds of every site, the per-layer and per-step seed arithmetic, the device step counter);
* the front-end projection (frontend.linear, frame_frontend folded and unfolded).

A wrong or mis-seeded mask at any site moves these quantities by about sqrt(2 p / (1 - p)) = 0.47 relative L2, far
outside every bound below, so the bounds separate "same mask" from "another mask" with a wide margin.

Tolerances are the project's own for the same quantities without dropout, unchanged: no quantity needed a margin over
its p = 0 bound.  Measured on an MI355X at p = 0.1 (whole encoder, worst over the cases and runs): fp32 y 2.6e-7, per-row
6.6e-7, dx 3.6e-7 against 1e-4 / 1e-3 / 1e-3; bf16 y 2.1e-3, per-row 4.0e-3, dx 2.7e-3, worst parameter gradient 1.2e-2
against 3e-2 / 8e-2 / 5e-2 / 5e-2.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import nn_conformer_for_speech_recognition_amd.conformer as cm
from nn_conformer_for_speech_recognition_amd import _lib, ops
from nn_conformer_for_speech_recognition_amd import frontend as fe
from nn_conformer_for_speech_recognition_amd.conformer import Conformer
from oracle import conformer as oc
from tests import dropout_hash as dh
from tests.test_gpu_attention import _ref, _ref_rel, _rel_case
from tests.test_gpu_conformer import ROWTOL, TOL, rel_err, row_max_err
from tests.test_gpu_frontfold import NAMES as FRONT_NAMES
from tests.test_gpu_frontfold import SHAPES as FRONT_SHAPES
from tests.test_gpu_frontfold import make as front_make
from tests.test_gpu_frontfold import run_fold

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.1
WIDE = (1 << 40) + 5
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def attn_mode():
    yield lambda m: _lib.call("cfm_attn_set_mode", m)
    _lib.call("cfm_attn_set_mode", 0)


@pytest.fixture
def restore_ln_pair():
    keep = cm.LN_PAIR
    yield
    cm.LN_PAIR = keep


# ------------------------------------------------------------------------------------------ attention core
@functools.lru_cache(maxsize=None)
def _attn_case(B, T, H, dk, lens, rel, seed):
    """inputs and the torch reference under the helper mask: computed once, shared by the modes, never changed"""
    g = torch.Generator().manual_seed(T + dk + H)
    if rel:
        qkv, pos, pu, pv, do, ln = _rel_case(B, T, H, dk, list(lens), T + H)
    else:
        qkv = torch.randn(B * T, 3 * H * dk, generator=g).to(DEV, BF)
        do = torch.randn(B * T, H * dk, generator=g).to(DEV, BF)
        ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
        pos = pu = pv = None
    keep = torch.from_numpy(dh.attn_keep(B, H, T, P, seed)).to(DEV)
    ks = dh.keep_scale(P)
    if rel:
        ref = _ref_rel(qkv, pos, pu, pv, ln, B, T, H, dk, do, keep=keep, keep_scale=ks)
    else:
        ref = _ref(qkv, ln, B, T, H, dk, do, keep=keep, keep_scale=ks)
    return (qkv, pos, pu, pv, do, ln), ref


def _check_attention(got, ref, B, T, H, dk, lens, tag):
    """the bounds of test_attention_vs_torch / test_rel_attention_vs_torch (p = 0): relative L2 1e-2 (o), 2e-2 (dQ, dK, dV
    each, and dpos), 3e-2 (du, dv); per valid row max |err| / max |ref| 5e-2 on o"""
    o, dqkv, dpos, dpu, dpv = got
    HD = H * dk
    err = {"o": rel_err(o.float(), ref[0])}
    for i, n in enumerate(("dQ", "dK", "dV")):
        err[n] = rel_err(dqkv.float()[:, i * HD:(i + 1) * HD], ref[1][:, i * HD:(i + 1) * HD])
    if dpos is not None:
        err["dpos"] = rel_err(dpos.float(), ref[2])
        err["du"] = rel_err(dpu, ref[3])
        err["dv"] = rel_err(dpv, ref[4])
    ob, rb = o.float().view(B, T, -1).cpu(), ref[0].view(B, T, -1).cpu()
    worst = 0.0
    for b, n in enumerate(lens):
        den = rb[b, :n].abs().amax(-1)
        ok = den > 0                                 # (a row whose every kept key was dropped is all zero)
        assert bool((ob[b, :n][~ok] == 0).all())
        if ok.any():
            worst = max(worst, ((ob[b, :n] - rb[b, :n]).abs().amax(-1)[ok] / den[ok]).max().item())
    err["o_row"] = worst
    print(f"ATTN p{P} {tag} {err}", flush=True)
    bound = {"o": 1e-2, "dQ": 2e-2, "dK": 2e-2, "dV": 2e-2, "dpos": 2e-2, "du": 3e-2, "dv": 3e-2, "o_row": 5e-2}
    for n, e in err.items():
        assert e < bound[n], (tag, n, e)


ABS_CASES = [(2, 130, 2, 64, (130, 77)), (3, 97, 2, 36, (97, 40, 1))]
REL_CASES = [(2, 150, 2, 64, (150, 111)), (3, 97, 2, 36, (97, 40, 1))]


@pytest.mark.parametrize("mode", [0, _lib.ATTN_MODE_TILED, _lib.ATTN_MODE_DQ_RECOMPUTE, "D"],
                         ids=["whole", "tiled", "dqrc", "rowdotD"])
@pytest.mark.parametrize("B,T,H,dk,lens", ABS_CASES)
@pytest.mark.parametrize("seed", [9, WIDE])
def test_attention_with_dropout_vs_torch(attn_mode, mode, B, T, H, dk, lens, seed):
    """"D": D = rowsum(dO o O) handed in, as the out-projection data-gradient GEMM's rowdot epilogue supplies it."""
    (qkv, _, _, _, do, ln), ref = _attn_case(B, T, H, dk, lens, False, seed)
    attn_mode(0 if mode == "D" else mode)
    o, lse = ops.attn_fwd(qkv, ln, B, T, H, dk, drop_p=P, seed=seed)
    D = None
    if mode == "D":
        D = (do.float() * o.float()).view(B, T, H, dk).sum(-1).permute(0, 2, 1).reshape(-1).contiguous()
    dqkv, _, _, _ = ops.attn_bwd(qkv, o, do, lse, ln, B, T, H, dk, drop_p=P, seed=seed, D=D)
    torch.cuda.synchronize()
    _check_attention((o, dqkv, None, None, None), ref, B, T, H, dk, lens, f"abs T{T} dk{dk} mode {mode} seed {seed}")


@pytest.mark.parametrize("mode", [0, _lib.ATTN_MODE_REL_SIMT, _lib.ATTN_MODE_REL_DQ_RECOMPUTE, "D"],
                         ids=["mfma", "simt", "dqrc", "rowdotD"])
@pytest.mark.parametrize("B,T,H,dk,lens", REL_CASES)
@pytest.mark.parametrize("seed", [9, WIDE])
def test_rel_attention_with_dropout_vs_torch(attn_mode, mode, B, T, H, dk, lens, seed):
    (qkv, pos, pu, pv, do, ln), ref = _attn_case(B, T, H, dk, lens, True, seed)
    attn_mode(0 if mode == "D" else mode)
    o, lse = ops.attn_fwd(qkv, ln, B, T, H, dk, pos, pu, pv, drop_p=P, seed=seed)
    D = ws = None
    if mode == "D":
        ws, D = ops.attn_ws(B, T, H, dk, True, qkv.device)
        D.copy_((do.float() * o.float()).view(B, T, H, dk).sum(-1).permute(0, 2, 1).reshape(-1))
    got = ops.attn_bwd(qkv, o, do, lse, ln, B, T, H, dk, pos, pu, pv, drop_p=P, seed=seed, D=D, ws=ws)
    torch.cuda.synchronize()
    _check_attention((o,) + tuple(got), ref, B, T, H, dk, lens, f"rel T{T} dk{dk} mode {mode} seed {seed}")


def test_rowdot_epilogue_d_feeds_attention_bwd_under_dropout():
    """The D the encoder really uses (bf16, dk 64): written by the rowdot epilogue of the GEMM that produces dO."""
    B, T, H, dk, lens, seed = 2, 130, 2, 64, (130, 77), 9
    (qkv, _, _, _, _, ln), _ = _attn_case(B, T, H, dk, lens, False, seed)
    g = torch.Generator().manual_seed(21)
    g4 = torch.randn(B * T, H * dk, generator=g).to(DEV, BF)
    w = (torch.randn(H * dk, H * dk, generator=g) * 0.05).to(DEV, BF)
    o, lse = ops.attn_fwd(qkv, ln, B, T, H, dk, drop_p=P, seed=seed)
    ws, D = ops.attn_ws(B, T, H, dk, False, qkv.device)
    do = ops.linear_dgrad(g4, w, wt=w.t().contiguous(), rowdot=(o, D, T))
    dqkv, _, _, _ = ops.attn_bwd(qkv, o, do, lse, ln, B, T, H, dk, drop_p=P, seed=seed, D=D, ws=ws)
    torch.cuda.synchronize()
    keep = torch.from_numpy(dh.attn_keep(B, H, T, P, seed)).to(DEV)
    ref = _ref(qkv, ln, B, T, H, dk, do, keep=keep, keep_scale=dh.keep_scale(P))
    _check_attention((o, dqkv, None, None, None), ref, B, T, H, dk, lens, "abs rowdot epilogue D")


# ------------------------------------------------------------------------------------------ one residual FFN module
@pytest.mark.parametrize("cd", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,d,ffn", [(385, 144, 576), (385, 512, 2048)])
def test_ffn_module_with_dropout_vs_fp64(M, d, ffn, cd):
    """y = x + 0.5 drop2(W2 drop1(silu(W1 xn + b1)) + b2) and its backward through the kernels exactly as
    conformer._ffn_fwd / _ffn_bwd launch them (seed for the SiLU output, seed + 1 for the module output; the backward
    regenerates mask 2 in cfm_scale_dropout and mask 1 in the data-gradient GEMM's act_grad epilogue), against torch
    autograd in fp64 under the two helper masks.  Bounds: test_gemm_epilogues' (1e-5 fp32, 1e-2 bf16) for every
    quantity."""
    seed = 1234
    g = torch.Generator().manual_seed(M + d)
    x = torch.randn(M, d, generator=g)
    xn = torch.randn(M, d, generator=g).to(cd)
    w1 = (torch.randn(ffn, d, generator=g) * d ** -0.5).to(cd)
    w2 = (torch.randn(d, ffn, generator=g) * ffn ** -0.5).to(cd)
    b1, b2 = torch.randn(ffn, generator=g) * 0.1, torch.randn(d, generator=g) * 0.1
    gy = torch.randn(M, d, generator=g)
    ks = dh.keep_scale(P)
    m1 = torch.from_numpy(dh.gemm_keep(M, ffn, P, seed)).double() * ks
    m2 = torch.from_numpy(dh.gemm_keep(M, d, P, seed + 1)).double() * ks
    leaves = [t.double().clone().requires_grad_() for t in (xn, w1, b1, w2, b2)]
    pre_r = leaves[0] @ leaves[1].T + leaves[2]
    h_r = torch.nn.functional.silu(pre_r) * m1
    y_r = x.double() + 0.5 * ((h_r @ leaves[3].T + leaves[4]) * m2)
    y_r.backward(gy.double())
    # the kernels, as _ffn_fwd / _ffn_bwd call them
    xd, xnd, w1d, w2d, b1d, b2d, gd = (t.to(DEV) for t in (x, xn, w1, w2, b1, b2, gy))
    pre = torch.empty(M, ffn, device=DEV, dtype=cd)
    h = ops.linear(xnd, w1d, b1d, act=ops.ACT_SILU, pre=pre, drop_p=P, seed=seed)
    y = ops.linear(h, w2d, b2d, drop_p=P, seed=seed + 1, out_scale=0.5, residual=xd, out_dtype=F32)
    g2 = ops.scale_dropout(gd, 0.5, P, seed + 1, 0, out_dtype=cd)
    dw2 = ops.linear_wgrad(g2, h)
    db2 = g2.float().sum(0)
    da = ops.linear_dgrad(g2, w2d, pre=pre, act_grad=True, drop_p=P, seed=seed, wt=w2d.t().contiguous())
    dw1 = ops.linear_wgrad(da, xnd)
    db1 = da.float().sum(0)
    dxn = ops.linear_dgrad(da, w1d, wt=w1d.t().contiguous())
    torch.cuda.synchronize()
    err = {"pre": rel_err(pre, pre_r.detach()), "h": rel_err(h, h_r.detach()), "y": rel_err(y, y_r.detach()),
           "dxn": rel_err(dxn, leaves[0].grad), "dW1": rel_err(dw1, leaves[1].grad), "db1": rel_err(db1, leaves[2].grad),
           "dW2": rel_err(dw2, leaves[3].grad), "db2": rel_err(db2, leaves[4].grad)}
    print(f"FFN p{P} M{M} d{d} {str(cd)[6:]} {err}", flush=True)
    tol = 1e-5 if cd == F32 else 1e-2
    for n, e in err.items():
        assert e < tol, (n, e)
    assert torch.equal(h == 0, (m1 == 0).to(DEV) | (pre == 0))


# ------------------------------------------------------------------------------------------ whole encoder
# The seed map, restated (not imported): layer i's base seed is seed + 100 i; its modules add ffn1 0, conv 10,
# attention 20, ffn2 30.  Within a module: the FFN's SiLU output draws under the module seed and its output under
# seed + 1; the attention probabilities under the module seed and the out-projection output under seed + 1; the conv
# module's output under the module seed.  GEMM-epilogue sites index their (B T, N) output by row-major position,
# attention by ((b H + h) T + i) T_even + j.  The public forward derives seed = (step 1000003 + 12345) & 0x7FFFFFFF
# from its step count; a bound device counter c turns every site's seed s into salted(s, c).
MODULE_OFFSET = {"ffn1": 0, "conv": 10, "attn": 20, "ffn2": 30}


def _provider(B, T, d, H, ffn, seed, counter=None):
    ks = dh.keep_scale(P)

    def sd(s):
        return s if counter is None else dh.salted(s, counter)

    def provider(site, shape):
        _, li, mod, what = site.split(".")
        s = seed + 100 * int(li) + MODULE_OFFSET[mod]
        if what == "probs":
            m = dh.attn_keep(B, H, T, P, sd(s))
        elif what == "act":
            m = dh.gemm_keep(B * T, ffn, P, sd(s)).reshape(B, T, ffn)
        elif mod == "conv":                                     # the oracle's conv dropout sees (B, d, T)
            m = dh.gemm_keep(B * T, d, P, sd(s)).reshape(B, T, d).transpose(0, 2, 1)
        else:                                                   # ffn*.out, attn.out
            m = dh.gemm_keep(B * T, d, P, sd(s + 1)).reshape(B, T, d)
        assert m.shape == tuple(shape), (site, m.shape, shape)
        return torch.from_numpy(np.ascontiguousarray(m)).double() * ks
    return provider


ENC_CASES = [
    # d, H, ffn, K, layers, B, T, lens, conv_first, pos, group_norm
    (144, 4, 576, 15, 2, 3, 130, (130, 129, 64), True, "none", False),
    (128, 2, 256, 15, 2, 2, 96, (96, 50), False, "rel", False),
    (512, 8, 2048, 31, 1, 2, 97, (97, 60), False, "none", False),       # dk 64: the rowdot-fused D runs in bf16
    (144, 4, 576, 15, 1, 2, 64, (64, 33), False, "none", True),
]
ENC_IDS = ["d144x2_convfirst", "d128x2_rel", "d512_dk64", "d144_groupnorm"]


@functools.lru_cache(maxsize=None)
def _enc_setup(case):
    d, H, ffn, K, L, B, T, lens, conv_first, pos, gn = case
    torch.manual_seed(7)
    ref = oc.ConformerRef(d, H, ffn, L, K, P, use_group_norm=gn, convolution_first=conv_first, pos_enc=pos)
    with torch.no_grad():
        for n, prm in ref.named_parameters():
            if n.endswith("bias"):
                prm.normal_(0, 0.05)
    ref = ref.double().train()
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    x = torch.randn(B, T, d)
    gy = torch.randn(B, T, d)
    return ref, sd0, x, gy


def _oracle_step(case, provider, steps=1):
    """the fp64 oracle from its initial state, `steps` training steps under provider(step) -> last step's
    (y, dx, {param: grad}, {buffer: value})"""
    ref, sd0, x, gy = _enc_setup(case)
    ref.load_state_dict(sd0)
    lens = torch.tensor(case[7])
    for k in range(steps):
        ref.set_mask_provider(provider(k))
        ref.zero_grad(set_to_none=True)
        xr = x.double().requires_grad_()
        y, _ = ref(xr, lens)
        y.backward(gy.double())
    ref.set_mask_provider(None)
    return (y.detach(), xr.grad, {n: p.grad.clone() for n, p in ref.named_parameters()},
            {n: b.clone() for n, b in ref.named_buffers() if "running" in n})


def _model(case, cd, p, fp8=False):
    d, H, ffn, K, L, B, T, lens, conv_first, pos, gn = case
    _, sd0, _, _ = _enc_setup(case)
    m = Conformer(d, H, ffn, L, K, p, use_group_norm=gn, convolution_first=conv_first, pos_enc=pos, compute_dtype=cd,
                  fp8=fp8)
    m.load_state_dict({k: v.float() for k, v in sd0.items()})
    return m.to(DEV).train()


def _errors(m, y, gx, want, lens):
    """every quantity test_encoder_vs_oracle compares -> {name: (error, kind)}, kind selecting its bound"""
    yr, gxr, gr, br = want
    err = {"y": (rel_err(y.detach(), yr), "y"), "y_row": (row_max_err(y.detach(), yr, lens), "row"),
           "dx": (rel_err(gx.reshape(gxr.shape), gxr), "g")}
    named = dict(m.named_parameters())
    for n, prm in named.items():
        assert prm.grad is not None, n
        if n.endswith("conv_module.sequential.2.bias") and not m.conformer_layers[0].use_group_norm:
            # train-mode BatchNorm right after the depthwise conv removes its bias: the true gradient is exactly 0, both
            # sides hold rounding noise (test_encoder_vs_oracle's exception, kept): noise-sized against the weight's
            wg = named[n.replace(".bias", ".weight")].grad
            assert prm.grad.norm() <= 1e-2 * wg.norm(), n
            continue
        err[n] = (rel_err(prm.grad, gr[n]), "g3" if "pos_bias" in n else "g")
    for n, b in m.named_buffers():
        if "running" in n:
            err[n] = (rel_err(b, br[n]), "y")
    return err


def _bound(cd, kind):
    tol_y, tol_g = TOL[cd]
    return {"y": tol_y, "row": ROWTOL[cd], "g": tol_g, "g3": 3 * tol_g}[kind]


def _assert_errors(err, cd, tag):
    worst = max(err, key=lambda n: err[n][0] / _bound(cd, err[n][1]))
    print(f"ENCODER p{P} {tag}: y {err['y'][0]:.3g} y_row {err['y_row'][0]:.3g} dx {err['dx'][0]:.3g} "
          f"worst/bound {worst} {err[worst][0]:.3g}/{_bound(cd, err[worst][1]):.3g}", flush=True)
    for n, (e, k) in err.items():
        assert e < _bound(cd, k), (tag, n, e, _bound(cd, k))


def _run_tokens(m, case, seed):
    B, T, d = case[5], case[6], case[0]
    _, _, x, gy = _enc_setup(case)
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).reshape(B * T, d).requires_grad_()
    lens = torch.tensor(case[7], dtype=torch.int32, device=DEV)
    y = m.forward_tokens(xd, lens, B, T, seed=seed)
    y.backward(gy.to(DEV).reshape(B * T, d))
    torch.cuda.synchronize()
    return y.view(B, T, d), xd.grad


@pytest.mark.parametrize("cd", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ENC_CASES, ids=ENC_IDS)
def test_encoder_with_dropout_vs_masked_oracle(restore_ln_pair, case, cd):
    """Conformer(dropout=0.1) in train mode against ConformerRef in fp64 under the helper masks of the restated seed
    map: outputs (relative L2 and per valid row), x.grad, every parameter gradient, the BatchNorm running statistics --
    test_encoder_vs_oracle's quantities and bounds (TOL, ROWTOL, 3x on pos_bias), its zero-gradient depthwise-bias
    exception kept.  Three runs: forward_tokens(seed=5); the public forward on a fresh model, first and second step
    (seed from the step count; running statistics after two updates); forward_tokens(seed=5) under a bound device
    counter of 2 against the salted masks.  Two-layer cases again with LN_PAIR off (the g2 of cfm_layernorm_bwd_drop
    instead of the pair kernel's)."""
    d, H, ffn, K, L, B, T, lens, conv_first, pos, gn = case
    tag = f"{ENC_IDS[ENC_CASES.index(case)]} {str(cd)[6:]}"
    # 1. explicit seed
    want = _oracle_step(case, lambda k: _provider(B, T, d, H, ffn, 5))
    default = cm.LN_PAIR
    for pair in ((True, False) if L > 1 else (default,)):
        cm.LN_PAIR = pair
        m = _model(case, cd, P)
        y, gx = _run_tokens(m, case, 5)
        _assert_errors(_errors(m, y, gx, want, lens), cd, f"{tag} seed 5 ln_pair {pair}")
    cm.LN_PAIR = default
    # 2. the public forward: two steps of a fresh model, seeds from the step count
    step_seed = [(k * 1000003 + 12345) & 0x7FFFFFFF for k in range(2)]
    _, _, x, gy = _enc_setup(case)
    m = _model(case, cd, P)
    ln = torch.tensor(lens, device=DEV)
    for k in range(2):
        m.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_()
        y, _ = m(xd, ln)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        want = _oracle_step(case, lambda j: _provider(B, T, d, H, ffn, step_seed[j]), steps=k + 1)
        _assert_errors(_errors(m, y, xd.grad, want, lens), cd, f"{tag} forward step {k}")
    # 3. a bound device step counter
    ctr = torch.full((1,), 2, dtype=torch.int64, device=DEV)
    m = _model(case, cd, P)
    _lib.call("cfm_rng_bind", _lib.ptr(ctr))
    try:
        y, gx = _run_tokens(m, case, 5)
    finally:
        torch.cuda.synchronize()
        _lib.call("cfm_rng_bind", None)
    want = _oracle_step(case, lambda k: _provider(B, T, d, H, ffn, 5, counter=2))
    _assert_errors(_errors(m, y, gx, want, lens), cd, f"{tag} seed 5 counter 2")


def test_fp8_encoder_with_dropout_vs_masked_oracle():
    """The fp8 forward (MX e4m3 FFN / QKV / out-projection GEMMs, bf16 backward) with dropout 0.1 under the same seed
    map: Conformer-L dims, rel-pos, against the masked fp64 oracle at test_conformer_fp8_forward_vs_fp32_oracle's
    bounds (relative L2 5e-2 output, 1e-1 input and parameter gradients, 3x on pos_bias; the exactly-zero depthwise-bias
    gradient left out as there)."""
    case = (512, 8, 2048, 31, 1, 2, 97, (97, 60), False, "rel", False)
    d, H, ffn, K, L, B, T, lens = case[:8]
    want = _oracle_step(case, lambda k: _provider(B, T, d, H, ffn, 5))
    m = _model(case, BF, P, fp8=True)
    y, gx = _run_tokens(m, case, 5)
    err = _errors(m, y, gx, want, lens)
    worst = max((n for n in err if n not in ("y", "y_row") and "running" not in n), key=lambda n: err[n][0])
    print(f"ENCODER p{P} fp8: y {err['y'][0]:.3g} dx {err['dx'][0]:.3g} worst gradient {worst} {err[worst][0]:.3g}",
          flush=True)
    for n, (e, k) in err.items():
        if n != "y_row":
            assert e < {"y": 5e-2, "g": 1e-1, "g3": 3e-1}[k], (n, e)


# ------------------------------------------------------------------------------------------ front-end projection
@pytest.mark.parametrize("cd", [F32, BF], ids=["fp32", "bf16"])
def test_frontend_linear_with_dropout_vs_fp64(cd):
    """frontend.linear(drop_p=0.2, seed=77): y = mask o (x W^T + b) * keep and its backward (the mask regenerated by
    cfm_scale_dropout) against fp64 under gemm_keep(M, N).  Bounds: test_gemm_layouts' 1e-5 fp32 / 1e-2 bf16."""
    M, K, N, p, seed = 97, 144, 64, 0.2, 77
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).to(cd)
    lin = torch.nn.Linear(K, N)
    gy = torch.randn(M, N, generator=g)
    mask = torch.from_numpy(dh.gemm_keep(M, N, p, seed)).double() * dh.keep_scale(p)
    wq = lin.weight.detach().to(cd).double()           # the GEMM reads the weight in the compute dtype
    leaves = [t.clone().requires_grad_() for t in (x.double(), wq, lin.bias.detach().double())]
    yr = (leaves[0] @ leaves[1].T + leaves[2]) * mask
    yr.backward(gy.double())
    lin = lin.to(DEV)
    xd = x.to(DEV).requires_grad_()
    y = fe.linear(xd, lin.weight, lin.bias, cd=cd, drop_p=p, seed=seed)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    err = {"y": rel_err(y.detach(), yr.detach()), "dx": rel_err(xd.grad, leaves[0].grad),
           "dW": rel_err(lin.weight.grad, leaves[1].grad), "db": rel_err(lin.bias.grad, leaves[2].grad)}
    print(f"FRONT linear p{p} {str(cd)[6:]} {err}", flush=True)
    assert torch.equal((y == 0).cpu(), mask == 0)
    tol = 1e-5 if cd == F32 else 1e-2
    for n, e in err.items():
        assert e < tol, (n, e)


def _front_reference(cs, proj, x, gy, mask):
    """tests/test_gpu_frontfold.py reference() with the projection's output masked: fp64 CPU"""
    import torch.nn.functional as F
    ps = [q.detach().double().clone().requires_grad_() for q in
          (cs.conv_sub_1.weight, cs.conv_sub_1.bias, cs.conv_sub_2.weight, cs.conv_sub_2.bias, proj.weight, proj.bias)]
    h = F.conv2d(x.double().unsqueeze(1), ps[0], ps[1], stride=2)
    h = F.conv2d(h, ps[2], ps[3], stride=2)
    B, C2, F2, T2 = h.shape
    y = F.linear(h.permute(0, 3, 2, 1).reshape(B * T2, F2 * C2), ps[4], ps[5]) * mask
    y.backward(gy.double())
    return y.detach(), [q.grad for q in ps]


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("cd", [F32, BF], ids=["fp32", "bf16"])
def test_frame_frontend_with_dropout_vs_fp64(cd, fold):
    """frame_frontend(drop_p=0.2, seed=77) at the smallest shape of test_fold_vs_fp64_composition, folded (one GEMM) and
    unfolded (conv kernels + projection GEMM), against the fp64 composition under gemm_keep(B T2, D).
    Bounds: the folded path's are test_fold_vs_fp64_composition's (fp32 2e-6 / 2e-5, bf16 hi + lo 4e-3 / 1e-2); the
    unfolded kernels have no fp64 bound of their own in that file, only test_fold_dropout_matches_unfolded_kernels'
    distance to the folded path (1e-5 / 1e-4 fp32, 2e-2 / 3e-2 bf16), so theirs is the sum of the two."""
    shape = min(FRONT_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3] * s[4] * s[5])
    p, seed = 0.2, 77
    cs, proj, x, (F2, T2) = front_make(*shape)
    B, D = shape[0], shape[5]
    gy = torch.randn(B * T2, D)
    mask = torch.from_numpy(dh.gemm_keep(B * T2, D, p, seed)).double() * dh.keep_scale(p)
    ref, rgrads = _front_reference(cs, proj, x, gy, mask)
    y, grads = run_fold(cs, proj, x, gy, cd, drop_p=p, seed=seed, fold=fold)
    tol_y, tol_g = (2e-6, 2e-5) if cd == F32 else (4e-3, 1e-2)
    if not fold:
        tol_y, tol_g = (tol_y + 1e-5, tol_g + 1e-4) if cd == F32 else (tol_y + 2e-2, tol_g + 3e-2)
    err = {"y": rel_err(y, ref)}
    err.update({n: rel_err(a, b) for n, a, b in zip(FRONT_NAMES, grads, rgrads)})
    print(f"FRONT frame p{p} {str(cd)[6:]} fold {fold} {err}", flush=True)
    assert torch.equal(y == 0, mask == 0)
    assert err.pop("y") < tol_y
    for n, e in err.items():
        assert e < tol_g, (n, e)
