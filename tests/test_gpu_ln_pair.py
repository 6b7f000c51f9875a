"""The fused LayerNorm pair at an encoder layer boundary (final_layer_norm of layer i, then the ffn1 LayerNorm of
layer i + 1): ops.layernorm_fwd_pair / layernorm_bwd_pair against the two-call path they replace and against torch
autograd, and the encoder with conformer.LN_PAIR on against off.

Bounds (relative L2 over the whole tensor):
  forward: y, z and both rows of statistics bit-identical to two ops.layernorm_fwd calls.
  backward, against the two-call path: dx < 1e-6 (y is recomputed from x and the products are contracted differently,
    so single fp32 roundings may differ: ten times the fp32 unit round-off, a tenth of test_layernorm's fp32 bound);
    the four parameter gradients < 1e-5; g2 bit-identical to ops.scale_dropout of the fused dx.
  backward, against torch autograd: test_layernorm's own bounds (1e-5 fp32, 1e-2 with bf16 gradients).
  encoder, LN_PAIR on against off: outputs bit-identical; the input gradient and every parameter gradient < 1e-5 in
    fp32 compute, < 1e-3 in bf16 compute (the rare bf16 re-roundings of the gradients g2 and the dgrad GEMMs carry)."""
import functools

import pytest
import torch

import nn_conformer_for_speech_recognition_amd.conformer as cm
from nn_conformer_for_speech_recognition_amd import _lib, ops
from nn_conformer_for_speech_recognition_amd.conformer import Conformer
from nn_conformer_for_speech_recognition_amd.ctc import ctc_head_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------- kernel level
@functools.lru_cache(maxsize=None)
def _case(D, M, dtype):
    """Inputs, the two-call results and torch autograd's gradients of one shape: computed once, shared, never changed."""
    g = torch.Generator().manual_seed(1000 * D + M)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    g1, b1 = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    g2, b2 = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    dz = torch.randn(M, D, generator=g).to(dtype)
    dres = torch.randn(M, D, generator=g)
    leaves = [t.clone().double().requires_grad_() for t in (x, g1, b1, g2, b2)]
    yr = torch.nn.functional.layer_norm(leaves[0], (D,), leaves[1], leaves[2], 1e-5)
    zr = torch.nn.functional.layer_norm(yr, (D,), leaves[3], leaves[4], 1e-5)
    torch.autograd.backward([zr, yr], [dz.double(), dres.double()])
    auto = [t.grad for t in leaves]
    dev = [t.to(DEV) for t in (x, g1, b1, g2, b2, dz, dres)]
    x_, g1_, b1_, g2_, b2_, dz_, dres_ = dev
    y, m1, r1 = ops.layernorm_fwd(x_, g1_, b1_, out_dtype=torch.float32)
    z, m2, r2 = ops.layernorm_fwd(y, g2_, b2_, out_dtype=dtype)
    dy, dg2, db2 = ops.layernorm_bwd(dz_, y, g2_, m2, r2, dres=dres_)
    dx, dg1, db1 = ops.layernorm_bwd(dy, x_, g1_, m1, r1)
    torch.cuda.synchronize()
    return dev, (y, z, m1, r1, m2, r2), (dx, dg1, db1, dg2, db2), auto


SHAPES = [(D, M) for D in (512, 256, 144) for M in (777, 5)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D,M", SHAPES)
def test_pair_forward_bit_identical_to_two_calls(D, M, dtype):
    (x, g1, b1, g2, b2, _, _), two, _, _ = _case(D, M, dtype)
    assert ops.layernorm_pair_ok(D, dtype)
    got = ops.layernorm_fwd_pair(x, g1, b1, g2, b2, out_dtype=dtype)
    assert got[1].dtype == dtype
    for name, a, b in zip(("y", "z", "mean1", "rstd1", "mean2", "rstd2"), got, two):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D,M", SHAPES)
def test_pair_backward_vs_two_calls_and_autograd(D, M, dtype, p):
    (x, g1, b1, g2, b2, dz, dres), (_, _, m1, r1, m2, r2), two, auto = _case(D, M, dtype)
    drop = (0.5, p, 4242, torch.bfloat16)
    dx, (dg1, db1), (dg2, db2), gout = ops.layernorm_bwd_pair(dz, dres, x, g1, b1, m1, r1, g2, m2, r2, drop=drop)
    err = {"dx": _rel(dx, two[0])}
    for name, a, b in zip(("dgamma1", "dbeta1", "dgamma2", "dbeta2"), (dg1, db1, dg2, db2), two[1:]):
        err[name] = _rel(a, b)
    ea = {name: _rel(a, b) for name, a, b in zip(("dx", "dgamma1", "dbeta1", "dgamma2", "dbeta2"),
                                                 (dx, dg1, db1, dg2, db2), auto)}
    print(f"LNPAIR D{D} M{M} {str(dtype)[6:]} p{p} vs two calls {err} vs autograd {ea}", flush=True)
    assert err["dx"] < 1e-6, err
    assert all(e < 1e-5 for n, e in err.items() if n != "dx"), err
    assert gout.dtype == torch.bfloat16
    assert torch.equal(gout, ops.scale_dropout(dx, 0.5, p, 4242, 0, out_dtype=torch.bfloat16))
    if p > 0:
        assert 0.05 < (gout == 0).float().mean().item() < 0.15
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert all(e < tol for e in ea.values()), ea


def test_pair_backward_deferred_partials_and_no_residual():
    """dgb NULL leaves the partial rows for the caller (the grouped column reduction's two tasks); dres may be absent."""
    D, M = 144, 777
    (x, g1, b1, g2, b2, dz, dres), (_, _, m1, r1, m2, r2), _, _ = _case(D, M, torch.bfloat16)

    class Side:
        rgroup = None

        def run(self, fn, *keep):
            fn()
    want = ops.layernorm_bwd_pair(dz, dres, x, g1, b1, m1, r1, g2, m2, r2)
    got = ops.layernorm_bwd_pair(dz, dres, x, g1, b1, m1, r1, g2, m2, r2, side=Side())
    assert got[3] is None and torch.equal(got[0], want[0])
    for a, b in zip(got[1] + got[2], want[1] + want[2]):
        assert torch.equal(a, b)
    y = ops.layernorm_fwd(x, g1, b1, out_dtype=torch.float32)[0]
    dy = ops.layernorm_bwd(dz, y, g2, m2, r2)[0]
    dx = ops.layernorm_bwd(dy, x, g1, m1, r1)[0]
    assert _rel(ops.layernorm_bwd_pair(dz, None, x, g1, b1, m1, r1, g2, m2, r2)[0], dx) < 1e-6


def test_pair_refuses_unsupported_width():
    x = torch.randn(8, 100, device=DEV)
    w = torch.ones(100, device=DEV)
    with pytest.raises(_lib.CfmError):
        ops.layernorm_fwd_pair(x, w, w, w, w)


# ---------------------------------------------------------------------------------------------- encoder level
def _encoder_run(d, H, ffn, layers, cd, p, passes=1):
    """One model, the same step with LN_PAIR on and off -> [(y, dx, {name: grad})] for on, off."""
    torch.manual_seed(3)
    B, T, K = 2, 37, 31
    m = Conformer(d, H, ffn, layers, K, dropout=p, compute_dtype=cd).to(DEV).train()
    with torch.no_grad():
        for n, prm in m.named_parameters():
            if n.endswith("bias"):
                prm.normal_(0, 0.05)
    x = torch.randn(B * T, d, device=DEV)
    gy = torch.randn(B * T, d, device=DEV)
    lens = torch.tensor([T, T - 9], dtype=torch.int32, device=DEV)
    out = []
    for on in (True, False):
        cm.LN_PAIR = on
        for prm in m.parameters():
            prm.grad = None
        xd = x.clone().requires_grad_()
        for k in range(passes):
            y = m.forward_tokens(xd, lens, B, T, seed=5 + k)
            y.backward(gy)
        torch.cuda.synchronize()
        out.append((y.detach(), xd.grad.clone(), {n: prm.grad.clone() for n, prm in m.named_parameters()}))
    return out


def _compare(on, off, cd, tag):
    tol = 1e-5 if cd == torch.float32 else 1e-3
    assert torch.equal(on[0], off[0])
    err = {"dx": _rel(on[1], off[1])}
    for n, g in on[2].items():
        if n.endswith("conv_module.sequential.2.bias"):
            # train-mode BatchNorm right after the depthwise conv removes that conv's bias: its true gradient is 0 and
            # both runs hold rounding noise (test_gpu_conformer.py), so the two are held together on the scale of the
            # depthwise weight gradient, which the same kernel produces
            scale = off[2][n.replace(".bias", ".weight")].double().norm().item()
            err[n] = (g.double() - off[2][n].double()).norm().item() / scale
        else:
            err[n] = _rel(g, off[2][n])
    worst = max(err, key=err.get)
    print(f"LNPAIR encoder {tag}: dx {err['dx']:.3g} worst {worst} {err[worst]:.3g}", flush=True)
    assert err[worst] < tol, (worst, err[worst])


@pytest.fixture
def restore_ln_pair():
    keep = cm.LN_PAIR
    yield
    cm.LN_PAIR = keep


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d,H,ffn,layers", [(144, 4, 576, 3), (512, 8, 2048, 2)], ids=["d144x3", "d512x2"])
def test_encoder_ln_pair_on_vs_off(restore_ln_pair, d, H, ffn, layers, cd, p):
    on, off = _encoder_run(d, H, ffn, layers, cd, p)
    _compare(on, off, cd, f"d{d} {str(cd)[6:]} p{p}")


@pytest.mark.parametrize("cd", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d,H,ffn,layers", [(144, 4, 576, 3), (512, 8, 2048, 2)], ids=["d144x3", "d512x2"])
def test_encoder_ln_pair_two_accumulated_backward_passes(restore_ln_pair, d, H, ffn, layers, cd):
    """.grad accumulates over two passes (fresh dropout masks each): the second pass finds .grad set, so no gradient is
    deferred to the grouped launches -- among them the ffn1 LayerNorm gradients the layer below now produces."""
    on, off = _encoder_run(d, H, ffn, layers, cd, 0.1, passes=2)
    _compare(on, off, cd, f"d{d} {str(cd)[6:]} two passes")


def test_encoder_ln_pair_is_what_runs(restore_ln_pair, monkeypatch):
    """With the switch on the boundary LayerNorms run fused (and only there); off, never."""
    calls = []
    real = ops.layernorm_fwd_pair
    monkeypatch.setattr(ops, "layernorm_fwd_pair", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m = Conformer(144, 4, 576, 3, 31).to(DEV).train()
    x = torch.randn(2 * 37, 144, device=DEV)
    lens = torch.tensor([37, 28], dtype=torch.int32, device=DEV)
    cm.LN_PAIR = True
    m.forward_tokens(x, lens, 2, 37, seed=1)
    assert len(calls) == 2
    cm.LN_PAIR = False
    m.forward_tokens(x, lens, 2, 37, seed=1)
    assert len(calls) == 2
    monkeypatch.setattr(cm, "RES_FUSE", True)
    cm.LN_PAIR = True
    m.forward_tokens(x, lens, 2, 37, seed=1)
    assert len(calls) == 2


def test_encoder_ln_pair_off_under_graph_capture(restore_ln_pair):
    """The two-call path stays capturable: a captured step with LN_PAIR off replays bit-identically to the eager one."""
    cm.LN_PAIR = False
    torch.manual_seed(0)
    B, T, d, V, U = 2, 37, 144, 24, 6
    model = Conformer(d, 4, 576, 3, 31, dropout=0.1).to(DEV).train()
    head = torch.nn.Linear(d, V).to(DEV)
    x = torch.randn(B * T, d, device=DEV)
    lens = torch.tensor([T, T - 9], dtype=torch.int32, device=DEV)
    tgt = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    tl = torch.tensor([U, 4], dtype=torch.int32, device=DEV)
    params = list(model.parameters()) + list(head.parameters())

    def step():
        y = model.forward_tokens(x, lens, B, T, seed=5)
        loss, _ = ctc_head_loss(y, head.weight, head.bias, tgt, lens, tl, B, T, zero_infinity=True)
        loss.backward()
        return loss

    def grads():
        return torch.cat([prm.grad.reshape(-1) for prm in params]).clone()

    def clear():
        for prm in params:
            prm.grad = None
    clear()
    want = (step().item(), grads())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture
        clear()
        step()
    torch.cuda.current_stream().wait_stream(side)
    clear()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert static.item() == want[0]
    assert torch.equal(grads(), want[1])
