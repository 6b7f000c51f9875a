"""The RNN-T loss on the device (csrc/rnnt.hip, transducer.rnnt_loss) against the fp64 restatement of tests/rnnt_ref.py.

Bounds:
  ll        |err| <= 1e-5 |ref| + 1e-6 against fp64 (the bound test_gpu_ctc_nbest holds the same state arithmetic to);
  gradient  the yardstick is the SAME formula in fp32 on the CPU: max |err| <= 2 max |err of the fp32 reference|
            + 1e-7 max |ref| per case (that test's rule);
  zeros     exact (bitwise +0) outside the valid cells t < T_b, u <= U_b and for utterances without frames.
Measured on the MI355X (worst error / bound per case): profiles/rnnt/errors.txt, DESIGN.md."""
import functools

import numpy as np
import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ops, transducer
from tests import rnnt_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = rr.CASES[name]
    return rr.reference(**c), rr.reference(**c, dtype=np.float32)


def _inputs(c, ids_dtype=torch.int64):
    return dict(x=torch.from_numpy(c["x"]).to(DEV), tg=torch.from_numpy(c["targets"]).to(DEV, ids_dtype),
                il=torch.tensor(c["ils"], dtype=torch.int32, device=DEV),
                tl=torch.tensor(c["tls"], dtype=torch.int32, device=DEV))


def _run(c, x=None, tg=None, il="case", tl="case", g=None, ids_dtype=torch.int64, **kw):
    """rnnt_loss(reduction='none') forward + backward -> (loss (B,), grad (B, T, U1, V)) device tensors."""
    d = _inputs(c, ids_dtype)
    x = (d["x"] if x is None else x).detach().requires_grad_()
    loss = transducer.rnnt_loss(x, d["tg"] if tg is None else tg, d["il"] if isinstance(il, str) else il,
                                d["tl"] if isinstance(tl, str) else tl, blank=c["blank"], reduction="none", **kw)
    loss.backward(torch.ones_like(loss) if g is None else g)
    return loss.detach(), x.grad


def _is_pos_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


@pytest.mark.parametrize("name", list(rr.CASES))
def test_cases_against_fp64(name):
    c = rr.CASES[name]
    ref, ref32 = _refs(name)
    B, T, U1, V = c["x"].shape
    loss_d, grad_d = _run(c)
    ll, grad = -loss_d.cpu().double().numpy(), grad_d.cpu().double().numpy()
    assert ll.shape == (B,) and grad.shape == (B, T, U1, V)
    fin = np.isfinite(ref["ll"])
    assert (ll[~fin] == -np.inf).all() and np.isfinite(ll[fin]).all()
    err = np.abs(ll[fin] - ref["ll"][fin])
    bound = 1e-5 * np.abs(ref["ll"][fin]) + 1e-6
    print(f"  {name} B {B} T {T} U1 {U1} V {V}: ll err {err.max():.3g}  bound {bound.min():.3g}")
    line = [f"ll {float((err / bound).max()):.4f}"]
    assert (err <= bound).all(), (name, err.max())
    e = np.abs(grad - ref["grad"]).max()
    e32 = np.abs(ref32["grad"] - ref["grad"]).max()
    bound = 2 * e32 + 1e-7 * np.abs(ref["grad"]).max()
    print(f"  {name}: grad err {e:.3g}  fp32 reference err {e32:.3g}  bound {bound:.3g}")
    line.append(f"grad {e:.3g} / {bound:.3g} = {e / bound:.4f}")
    print(f"  RATIOS {name}: " + "; ".join(line))
    assert e <= bound, (name, e, e32, bound)
    # exact zeros outside the valid cells
    for b in range(B):
        assert _is_pos_zero(grad_d[b, c["ils"][b]:]) and _is_pos_zero(grad_d[b, :, c["tls"][b] + 1:]), (name, b)
        if c["ils"][b] == 0:
            assert _is_pos_zero(grad_d[b])
        else:
            assert float(grad_d[b].abs().max()) > 1e-3


def test_poisoned_padding_garbage_ids_and_lengths_are_bit_identical():
    c = rr.CASES["ragged_T_0_and_1"]
    B, T, U1, V = c["x"].shape
    d = _inputs(c)
    base = _run(c)
    assert float(base[1].abs().max()) > 1e-3
    nan = d["x"].clone()
    for b, (tb, ub) in enumerate(zip(c["ils"], c["tls"])):
        nan[b, tb:] = float("nan")
        nan[b, :, ub + 1:] = float("nan")
    pos = torch.arange(U1 - 1, device=DEV)[None, :]
    past = pos >= d["tl"][:, None]
    wide = torch.full((B, U1 + 6), 77, dtype=torch.int64, device=DEV)
    wide[:, :U1 - 1] = d["tg"]
    big = torch.full((B, T, U1, 2 * V), 50.0, device=DEV)
    big[..., :V] = d["x"]
    variants = {
        "NaN outside the valid cells": _run(c, x=nan),
        "garbage ids past U_b": _run(c, tg=torch.where(past, torch.full_like(d["tg"], 123456), d["tg"])),
        "negative garbage ids past U_b": _run(c, tg=torch.where(past, torch.full_like(d["tg"], -9), d["tg"])),
        "int32 ids": _run(c, ids_dtype=torch.int32),
        "wider, strided targets": _run(c, tg=wide[:, :U1 + 2]),
        "host lengths": _run(c, il=list(c["ils"]), tl=list(c["tls"])),
        "host tensors": _run(c, il=torch.tensor(c["ils"]), tl=torch.tensor(c["tls"])),
        "non-contiguous logits": _run(c, x=big[..., :V]),
    }
    for what, got in variants.items():
        assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]), what
    # lengths past the clamps are the clamps; None is the full lattice
    full = dict(c, ils=[T] * B, tls=[U1 - 1] * B)
    want = _run(full)
    for what, got in {
        "None": _run(full, il=None, tl=None),
        "past the clamps": _run(full, il=torch.tensor([T + 5, T, 2 ** 30, T + 1], device=DEV),
                                tl=torch.tensor([U1 + 7, U1 - 1, 2 ** 30, U1], device=DEV)),
    }.items():
        assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), what
    neg = _run(full, il=torch.tensor([-3, T, T, T], device=DEV), tl=torch.tensor([U1 - 1, -2, U1 - 1, U1 - 1], device=DEV))
    zero = _run(dict(full, ils=[0, T, T, T], tls=[U1 - 1, 0, U1 - 1, U1 - 1]))
    assert torch.equal(neg[0], zero[0]) and torch.equal(neg[1], zero[1])
    # a label past V - 1 inside the length is clamped to V - 1: a wrong answer, never an access outside the row
    bad = d["tg"].clone()
    bad[3, 0] = 10 ** 6
    clamped = d["tg"].clone()
    clamped[3, 0] = V - 1
    a, k = _run(c, tg=bad), _run(c, tg=clamped)
    assert torch.equal(a[0], k[0]) and torch.equal(a[1], k[1])
    # other dtypes are cast to fp32; the incoming gradient scales each utterance's rows
    x64 = d["x"].double().requires_grad_()
    l64 = transducer.rnnt_loss(x64, d["tg"], d["il"], d["tl"], reduction="none")
    l64.backward(torch.ones_like(l64))
    assert l64.dtype == torch.float32 and torch.equal(l64.detach(), base[0])
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float(), base[1])
    g = torch.tensor([1.0, -2.0, 0.5, 3.0], device=DEV)
    assert torch.allclose(_run(c, g=g)[1], base[1] * g[:, None, None, None], rtol=1e-6, atol=0)


def test_guard_regions_survive():
    c = rr.CASES["U1_9_T17_V1024"]
    d = _inputs(c, ids_dtype=torch.int32)
    B, T, U1, V = c["x"].shape
    G, POISON = 64, -777.0
    want = _run(c)
    bufs = {k: torch.full((n + 2 * G,), POISON, device=DEV) for k, n in (("ll", B), ("grad", B * T * U1 * V))}
    mid = {k: v[G:v.numel() - G] for k, v in bufs.items()}
    nb = _lib.size_call("cfm_rnnt_ws_bytes", B, T, U1)
    cells = B * (T + U1 - 1) * U1
    assert nb % 16 == 0 and nb >= 24 * cells + 8 * B + 4 * B * T * U1
    ws = torch.full((nb // 4 + 2 * G,), POISON, device=DEV)      # (the poison also stands for uninitialised cells)
    p = _lib.ptr
    head = (p(d["x"]), p(d["tg"]), U1 - 1, p(d["il"]), p(d["tl"]), B, T, U1, V, c["blank"])
    _lib.call("cfm_rnnt_loss_fwd", *head, p(mid["ll"]), p(ws[G:]), _lib.stream())
    g = torch.ones(B, device=DEV)
    _lib.call("cfm_rnnt_loss_bwd", *head, p(ws[G:]), p(g), p(mid["grad"]), _lib.stream())
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v[:G] == POISON).all()) and bool((v[-G:] == POISON).all()), k
    assert bool((ws[:G] == POISON).all()) and bool((ws[G + nb // 4:] == POISON).all())
    assert torch.equal(-mid["ll"], want[0]) and torch.equal(mid["grad"], want[1].reshape(-1))


@pytest.mark.parametrize("name", ["U1_9_T17_V1024", "U1_257_T17_V2"])
def test_determinism_and_graph_replay(name):
    c = rr.CASES[name]
    d = _inputs(c, ids_dtype=torch.int32)
    U = c["targets"].shape[1]
    g = torch.ones(len(c["ils"]), device=DEV)
    first, again = _run(c), _run(c)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])

    def both():
        ll, ws = ops.rnnt_loss_fwd(d["x"], d["tg"], U, d["il"], d["tl"], c["blank"])
        return ll, ops.rnnt_loss_bwd(d["x"], d["tg"], U, d["il"], d["tl"], c["blank"], ws, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = both()
    for _ in range(2):
        for o in static:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(-static[0], first[0]) and torch.equal(static[1], first[1])


def test_no_host_synchronisation():
    c = rr.CASES["ragged_U_0_and_Umax"]
    d = _inputs(c)
    x = d["x"].clone().requires_grad_()
    transducer.rnnt_loss(x, d["tg"], d["il"], d["tl"]).backward()          # (warm-up: allocator, modules)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = transducer.rnnt_loss(x, d["tg"], d["il"], d["tl"], reduction="mean", zero_infinity=True)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss))


def test_reductions_and_zero_infinity():
    c = rr.CASES["ragged_T_0_and_1"]
    ref, _ = _refs("ragged_T_0_and_1")
    d = _inputs(c)
    none, grad = _run(c)
    assert float(none[0]) == np.inf and bool(torch.isfinite(none[1:]).all())
    zi, grad_zi = _run(c, zero_infinity=True)
    assert float(zi[0]) == 0.0 and torch.equal(zi[1:], none[1:]) and torch.equal(grad, grad_zi)
    for red, want in (("sum", zi.sum()), ("mean", zi.mean())):
        x = d["x"].clone().requires_grad_()
        got = transducer.rnnt_loss(x, d["tg"], d["il"], d["tl"], reduction=red, zero_infinity=True)
        assert got.shape == () and torch.equal(got, want), red
        got.backward()
        scale = 1.0 if red == "sum" else 1.0 / len(c["ils"])
        assert torch.allclose(x.grad, grad * scale, rtol=1e-6, atol=0), red
    assert abs(float(zi.mean()) - float(-ref["ll"][1:].sum() / 4)) <= 1e-5 * abs(ref["ll"][1:].sum())
    module = transducer.RNNTLoss(reduction="sum", zero_infinity=True)
    assert torch.equal(module(d["x"], d["tg"], d["il"], d["tl"]), zi.sum())
    # without zero_infinity the infinite loss stays in the reductions; its gradient is zero all the same
    assert float(transducer.rnnt_loss(d["x"], d["tg"], d["il"], d["tl"], reduction="mean")) == np.inf


def test_error_codes():
    B, T, U1, V = 2, 3, 4, 5
    x = torch.zeros(B, T, U1, V, device=DEV)
    tg = torch.ones(B, U1 - 1, dtype=torch.int32, device=DEV)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    tl = torch.full((B,), U1 - 1, dtype=torch.int32, device=DEV)
    ll = torch.zeros(B, device=DEV)
    gl = torch.ones(B, device=DEV)
    dx = torch.full((B, T, U1, V), 5.0, device=DEV)
    ws = torch.zeros(_lib.size_call("cfm_rnnt_ws_bytes", B, T, U1) // 4 + 2, device=DEV)
    assert ws.data_ptr() % 8 == 0
    p = _lib.ptr

    def fwd(x_=p(x), tg_=p(tg), ldt=U1 - 1, il_=p(il), tl_=p(tl), B_=B, T_=T, U1_=U1, V_=V, blank=0, ll_=p(ll),
            ws_=p(ws)):
        _lib.call("cfm_rnnt_loss_fwd", x_, tg_, ldt, il_, tl_, B_, T_, U1_, V_, blank, ll_, ws_, _lib.stream())

    def bwd(x_=p(x), tg_=p(tg), ldt=U1 - 1, il_=p(il), tl_=p(tl), B_=B, T_=T, U1_=U1, V_=V, blank=0, ws_=p(ws),
            gl_=p(gl), dx_=p(dx)):
        _lib.call("cfm_rnnt_loss_bwd", x_, tg_, ldt, il_, tl_, B_, T_, U1_, V_, blank, ws_, gl_, dx_, _lib.stream())

    fwd()
    bwd()
    for f in (fwd, bwd):
        for kw in (dict(B_=0), dict(T_=0), dict(U1_=0), dict(V_=0), dict(T_=-1), dict(ldt=U1 - 2)):
            with pytest.raises(_lib.CfmError, match=r"\(-2\).*bad shape"):
                f(**kw)
        for kw in (dict(x_=None), dict(tg_=None), dict(il_=None), dict(tl_=None), dict(ws_=None)):
            with pytest.raises(_lib.CfmError, match=r"\(-1\).*null pointer"):
                f(**kw)
        for blank in (-1, V):
            with pytest.raises(_lib.CfmError, match=r"\(-1\).*blank out of range"):
                f(blank=blank)
        with pytest.raises(_lib.CfmError, match=r"\(-5\).*1023 labels"):
            f(U1_=1025, ldt=1024)
        with pytest.raises(_lib.CfmError, match=r"\(-5\).*V must be >= 2"):
            f(V_=1)
        with pytest.raises(_lib.CfmError, match=r"\(-4\).*8-byte"):
            f(ws_=p(ws) + 4)
    with pytest.raises(_lib.CfmError, match=r"\(-1\).*null pointer"):
        fwd(ll_=None)
    for kw in (dict(gl_=None), dict(dx_=None)):
        with pytest.raises(_lib.CfmError, match=r"\(-1\).*null pointer"):
            bwd(**kw)
    torch.cuda.synchronize()
    assert _lib.size_call("cfm_rnnt_ws_bytes", 0, T, U1) == 0 and _lib.size_call("cfm_rnnt_ws_bytes", B, T, 0) == 0
    # no labels at all: targets may be NULL
    x1 = torch.zeros(B, T, 1, V, device=DEV)
    fwd(x_=p(x1), tg_=None, ldt=0, U1_=1)
    torch.cuda.synchronize()
    assert torch.allclose(ll, torch.full((B,), -T * float(np.log(V)), device=DEV))


def test_arguments():
    x = torch.zeros(2, 3, 4, 5, device=DEV)
    tg = torch.ones(2, 3, dtype=torch.int64, device=DEV)
    assert transducer.RNNT_MAX_LABELS == 1023
    transducer.rnnt_loss(x, tg)
    transducer.rnnt_loss(x, tg.cpu(), [3, 2], [3, 0])
    transducer.rnnt_loss(x, [[1, 2, 3], [3, 2, 1]])
    with pytest.raises(ValueError, match="reduction"):
        transducer.rnnt_loss(x, tg, reduction="batchmean")
    with pytest.raises(ValueError, match="blank"):
        transducer.rnnt_loss(x, tg, blank=5)
    with pytest.raises(RuntimeError):
        transducer.rnnt_loss(x.cpu(), tg)
    with pytest.raises(RuntimeError):
        transducer.rnnt_loss(x.long(), tg)
    with pytest.raises(ValueError):
        transducer.rnnt_loss(x[0], tg)
    with pytest.raises(ValueError):
        transducer.rnnt_loss(x[..., :1], tg)
    with pytest.raises(ValueError, match="targets"):
        transducer.rnnt_loss(x, tg[:, :2])
    with pytest.raises(ValueError, match="targets"):
        transducer.rnnt_loss(x, tg[:1])
    with pytest.raises(TypeError):
        transducer.rnnt_loss(x, tg.float())
    with pytest.raises(ValueError, match="logit_lengths"):
        transducer.rnnt_loss(x, tg, [3, 4], [3, 3])
    with pytest.raises(ValueError, match="target_lengths"):
        transducer.rnnt_loss(x, tg, [3, 3], [4, 3])
    with pytest.raises(ValueError):
        transducer.rnnt_loss(x, tg, [3], [3, 3])
    with pytest.raises(ValueError, match="1023"):
        transducer.rnnt_loss(torch.zeros(1, 1, 1025, 2, device=DEV), torch.ones(1, 1024, dtype=torch.int64, device=DEV))


def test_one_step_along_the_gradient_raises_the_likelihood():
    B, T, U1, V = 2, 94, 21, 1024
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((B, T, U1, V)).astype(np.float32)).to(DEV).requires_grad_()
    tg = torch.from_numpy(rng.integers(1, V, (B, U1 - 1))).to(DEV)
    il, tl = torch.tensor([T, 71], device=DEV), torch.tensor([U1 - 1, 13], device=DEV)
    loss = transducer.rnnt_loss(x, tg, il, tl, reduction="none")
    loss.sum().backward()
    assert bool(torch.isfinite(loss).all()) and float(loss.detach().min()) > 100
    stepped = (x - 1.0 * x.grad).detach()
    after = transducer.rnnt_loss(stepped, tg, il, tl, reduction="none")
    assert bool((after < loss - 0.1).all()), (loss.tolist(), after.tolist())
