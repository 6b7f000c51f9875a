"""The n-best CTC likelihood and the expected risk over it on the device (csrc/ctc_nbest.hip, ctc.nbest_log_likelihood,
ctc.expected_risk_loss, ctc.mwer_loss) against the fp64 restatement of tests/ctc_nbest_ref.py.

Bounds:
  ll            |err| <= 1e-5 |ref| + 1e-6 against fp64 (the bound test_gpu_ctc holds the same recursion to), and the
                same against -ctc.ctc_loss(reduction='none') of the problem expanded to B N rows;
  post, loss,   these amplify ll's absolute error through the softmax over n, so the yardstick is the SAME computation
  gradient      in fp32 torch on the CPU: max |err| <= 2 max |err of the fp32 reference| + 1e-7 max |ref| per case;
  zeros         exact (bitwise +0): frames t >= T_b, classes in no live hypothesis other than the blank, utterances
                with fewer than two live hypotheses or equal risks.
Measured on the MI355X (worst error / bound per case): profiles/mwer/errors.txt, DESIGN.md §8."""
import functools

import numpy as np
import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ctc, ops
from tests import ctc_nbest_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("ll", "post", "loss", "grad")


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = nr.CASES[name]
    return nr.reference(**c), nr.reference(**c, dtype=torch.float32)


def _inputs(c, ids_dtype=torch.int64, fill=-1):
    ids, lens = nr.pad_hyps(c["hyps"], width=c["max_labels"], fill=fill)
    return dict(x=torch.from_numpy(c["x"]).to(DEV), ids=ids.to(DEV, ids_dtype), lens=lens.to(DEV),
                il=torch.tensor(c["ils"], dtype=torch.int32, device=DEV),
                risk=torch.tensor(c["risks"], dtype=torch.float32, device=DEV))


def _run(c, x=None, ids=None, lens="case", il="case", risk=None, batch_first=True, g=None, **kw):
    """expected_risk_loss forward + backward -> (ll, post, loss, grad) device tensors (grad in batch-major)."""
    d = _inputs(c, **kw)
    x = (d["x"] if x is None else x).detach().requires_grad_()
    out = ctc.expected_risk_loss(x, d["ids"] if ids is None else ids, d["lens"] if isinstance(lens, str) else lens,
                                 d["risk"] if risk is None else risk, d["il"] if isinstance(il, str) else il,
                                 blank=c["blank"], batch_first=batch_first, max_labels=c["max_labels"])
    (out.loss.sum() if g is None else (out.loss * g).sum()).backward()
    grad = x.grad if batch_first else x.grad.transpose(0, 1)
    return out.ll, out.post, out.loss, grad


def _is_pos_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _live_classes(c, ref, b):
    return {c["blank"]} | {v for h, l in zip(c["hyps"][b], ref["ll"][b]) if h is not None and np.isfinite(l) for v in h}


@pytest.mark.parametrize("name", list(nr.CASES))
def test_cases_against_fp64(name):
    c = nr.CASES[name]
    ref, ref32 = _refs(name)
    B, T, V = c["x"].shape
    N = len(c["hyps"][0])
    ll, post, loss, grad = (t.detach().cpu().double().numpy() for t in _run(c))
    assert ll.shape == (B, N) and post.shape == (B, N) and loss.shape == (B,) and grad.shape == (B, T, V)
    # ll against fp64, and against the loss kernels on the expanded problem
    fin = np.isfinite(ref["ll"])
    assert (ll[~fin] == -np.inf).all() and np.isfinite(ll[fin]).all()
    err = np.abs(ll[fin] - ref["ll"][fin])
    bound = 1e-5 * np.abs(ref["ll"][fin]) + 1e-6
    assert (err <= bound).all(), (name, err.max())
    d = _inputs(c)
    ok = (d["lens"] >= 0) & (d["lens"] <= (c["max_labels"] if c["max_labels"] is not None else d["ids"].shape[-1]))
    nll = ctc.ctc_loss(d["x"].repeat_interleave(N, 0), d["ids"].clamp(min=1).reshape(B * N, -1),
                       d["il"].clamp(min=1).repeat_interleave(N), d["lens"].clamp(min=0).reshape(-1), blank=c["blank"],
                       reduction="none", batch_first=True)
    other = torch.where(ok.reshape(-1), -nll, torch.full_like(nll, -np.inf)).cpu().double().numpy().reshape(B, N)
    rows = np.array(c["ils"])[:, None] > 0                         # (an utterance without frames has no loss to compare)
    assert (other[~fin & rows] == -np.inf).all()
    assert (np.abs(ll[fin & rows] - other[fin & rows]) <= 1e-5 * np.abs(other[fin & rows]) + 1e-6).all(), name
    line = [f"ll {float((err / bound).max()):.4f}"]
    # post, loss, gradient: twice the fp32 CPU computation's own error
    for key, got in (("post", post), ("loss", loss), ("grad", grad)):
        e = np.abs(got - ref[key]).max()
        e32 = np.abs(ref32[key] - ref[key]).max()
        bound = 2 * e32 + 1e-7 * np.abs(ref[key]).max()
        line.append(f"{key} {e:.3g} / {bound:.3g} = {e / bound if bound > 0 else 0.0:.4f}")
        print(f"  {name} B {B} T {T} V {V} N {N}: {key} err {e:.3g}  fp32 reference err {e32:.3g}  bound {bound:.3g}")
        assert e <= bound, (name, key, e, e32, bound)
    print(f"  RATIOS {name}: " + "; ".join(line))
    # exact zeros
    g = _run(c)[3]
    for b in range(B):
        assert _is_pos_zero(g[b, c["ils"][b]:]), (name, b)
        dead = [v for v in range(V) if v not in _live_classes(c, ref, b)]
        assert _is_pos_zero(g[b][:, dead]), (name, b)
        if np.isfinite(ref["ll"][b]).sum() < 2:
            assert _is_pos_zero(g[b]) and loss[b] == 0, (name, b)


def test_nbest_log_likelihood_is_the_forward_without_risk():
    c = nr.CASES["N16_missing_identical"]
    d = _inputs(c)
    ll, post = ctc.nbest_log_likelihood(d["x"], d["ids"], d["lens"], d["il"])
    want = _run(c)
    assert torch.equal(ll, want[0]) and torch.equal(post, want[1]) and not ll.requires_grad
    assert torch.equal(ll[0, 0], ll[0, 1]) and torch.equal(post[0, 0], post[0, 1])      # two identical hypotheses


def test_n1_and_equal_risks_give_exact_zeros():
    c = dict(nr.CASES["prefetch_block"])
    c1 = dict(c, hyps=[hb[:1] for hb in c["hyps"]], risks=[rb[:1] for rb in c["risks"]])
    ll, post, loss, grad = _run(c1)
    assert _is_pos_zero(loss) and _is_pos_zero(grad) and bool((post == 1).all()) and bool(torch.isfinite(ll).all())
    for r in (0.1, 3.0, -7.3):
        eq = dict(c, risks=[[r] * len(rb) for rb in c["risks"]])
        ll, post, loss, grad = _run(eq)
        assert _is_pos_zero(loss) and _is_pos_zero(grad)
    c16 = nr.CASES["N16_missing_identical"]
    eq = dict(c16, risks=[[0.3] * 16] * 2)
    assert _is_pos_zero(_run(eq)[3])


def test_layouts_and_poisoned_padding_are_bit_identical():
    c = nr.CASES["ragged_T_0_and_1"]
    B, T, V = c["x"].shape
    d = _inputs(c)
    base = _run(c)
    assert float(base[3].abs().max()) > 1e-3
    big = torch.full((2 * B, T, V), 50.0, device=DEV)
    big[::2] = d["x"]
    nan = d["x"].clone()
    for b, tb in enumerate(c["ils"]):
        nan[b, tb:] = float("nan")
    ids_garbage = nr.pad_hyps(c["hyps"], fill=123456)[0].to(DEV)
    g = torch.tensor([1.0, -2.0, 0.5, 3.0], device=DEV)
    variants = {
        "time-major": _run(c, x=d["x"].transpose(0, 1).contiguous(), batch_first=False),
        "strided batch": _run(c, x=big[::2]),
        "int32 ids": _run(c, ids_dtype=torch.int32),
        "host lengths": _run(c, lens=nr.pad_hyps(c["hyps"])[1].tolist(), il=list(c["ils"])),
        "host tensors": _run(c, lens=nr.pad_hyps(c["hyps"])[1], il=torch.tensor(c["ils"])),
        "NaN past T_b": _run(c, x=nan),
        "garbage ids": _run(c, ids=ids_garbage),
        "negative garbage ids": _run(c, fill=-9),
    }
    for what, got in variants.items():
        for f, a, k in zip(NAMES, base, got):
            assert torch.equal(a, k), (what, f)
    # None lengths: every utterance T long, every hypothesis L long
    full = dict(c, ils=[T] * B, hyps=[[[1, 2, 3], [3, 2, 1], [1, 3, 1]]] * B)
    want = _run(full)
    got = _run(full, lens=None, il=None)
    for f, a, k in zip(NAMES, want, got):
        assert torch.equal(a, k), f
    # the incoming gradient scales each utterance's rows
    scaled = _run(c, g=g)
    assert torch.allclose(scaled[3], base[3] * g[:, None, None], rtol=1e-6, atol=0)


def test_guard_regions_survive():
    c = nr.CASES["V1024_N5"]
    d = _inputs(c, ids_dtype=torch.int32)
    B, T, V = c["x"].shape
    N, G, POISON = 5, 64, -777.0
    ml = d["ids"].shape[-1]
    want = _run(c)
    bufs = {k: torch.full((n + 2 * G,), POISON, device=DEV) for k, n in
            (("ll", B * N), ("post", B * N), ("loss", B), ("grad", B * T * V))}
    mid = {k: v[G:v.numel() - G] for k, v in bufs.items()}
    nb = _lib.size_call("cfm_ctc_nbest_ws_bytes", B, T, N, ml)
    ws = torch.full((nb // 4 + 2 * G,), POISON, device=DEV)
    p = _lib.ptr
    hl = d["lens"].to(torch.int32).reshape(-1).contiguous()
    head = (p(d["x"]), T * V, V, p(d["il"]), B, T, V, p(d["ids"]), ml, p(hl), N, ml, 0)
    _lib.call("cfm_ctc_nbest_fwd", *head, p(d["risk"].reshape(-1)), p(mid["ll"]), p(mid["post"]), p(mid["loss"]),
              p(ws[G:]), _lib.stream())
    g = torch.ones(B, device=DEV)
    _lib.call("cfm_ctc_nbest_bwd", *head, p(ws[G:]), p(g), 1, p(mid["grad"]), T * V, V, _lib.stream())
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v[:G] == POISON).all()) and bool((v[-G:] == POISON).all()), k
    assert bool((ws[:G] == POISON).all()) and bool((ws[G + nb // 4:] == POISON).all())
    for k, w in zip(NAMES, want):
        assert torch.equal(mid[k], w.reshape(-1)), k


def test_determinism_and_graph_replay():
    c = nr.CASES["V1024_N5"]
    d = _inputs(c, ids_dtype=torch.int32)
    hl = d["lens"].to(torch.int32).reshape(-1).contiguous()
    risk = d["risk"].reshape(-1).contiguous()
    ml = d["ids"].shape[-1]
    g = torch.ones(len(c["ils"]), device=DEV)
    first, again = _run(c), _run(c)
    for f, a, k in zip(NAMES, first, again):
        assert torch.equal(a, k), f

    def both():
        ll, post, loss, ws = ops.ctc_nbest_fwd(d["x"], d["il"], d["ids"].reshape(-1, ml), ml, hl, 5, ml, 0, risk)
        return ll, post, loss, ops.ctc_nbest_bwd(d["x"], d["il"], d["ids"].reshape(-1, ml), ml, hl, 5, ml, 0, ws, g)

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
        for f, a, k in zip(NAMES, first, static):
            assert torch.equal(a, k), f


def _mwer_inputs(seed=3, B=3, T=20, V=8):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * 2).astype(np.float32)).to(DEV)
    targets = torch.tensor(rng.integers(1, V, (B, 6)), device=DEV)
    return x, targets, torch.tensor([T, T - 5, 9], device=DEV), torch.tensor([6, 4, 0], device=DEV)


def test_no_host_synchronisation():
    c = nr.CASES["N16_missing_identical"]
    d = _inputs(c)
    x = d["x"].clone().requires_grad_()
    xm, targets, il, tl = _mwer_inputs()
    xm.requires_grad_()
    ctc.mwer_loss(xm, targets, il, tl, nbest=4, beam_size=8)[0].sum().backward()      # (warm-up: allocator, modules)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ctc.expected_risk_loss(x, d["ids"], d["lens"], d["risk"], d["il"])
        out.loss.sum().backward()
        loss, ed, post = ctc.mwer_loss(xm, targets, il, tl, nbest=4, beam_size=8)
        loss.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss).all())


def test_arguments():
    x = torch.zeros(2, 8, 5, device=DEV)
    il = torch.tensor([8, 8], dtype=torch.int32, device=DEV)
    ids = torch.ones(2, 3, 4, dtype=torch.int32, device=DEV)
    lens = torch.full((2, 3), 4, dtype=torch.int32, device=DEV)
    risk = torch.zeros(2, 3, device=DEV)
    ctc.expected_risk_loss(x, ids, lens, risk)
    for n in (0, 129):
        many = torch.ones(2, n, 4, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="N must be"):
            ctc.nbest_log_likelihood(x, many, None)
        hl = torch.ones(max(2 * n, 1), dtype=torch.int32, device=DEV)
        with pytest.raises(_lib.CfmError, match=r"\(-1\).*N must be >= 1" if n == 0 else r"\(-5\).*N must be <= 128"):
            ops.ctc_nbest_fwd(x, il, many.reshape(-1, 4), 4, hl, n, 4, 0)
    long = torch.ones(2, 3, 512, dtype=torch.int32, device=DEV)
    xl = torch.zeros(2, 530, 5, device=DEV)
    with pytest.raises(ValueError, match="max_labels"):
        ctc.nbest_log_likelihood(xl, long, None, max_labels=512)
    with pytest.raises(_lib.CfmError, match=r"\(-5\).*511"):
        ops.ctc_nbest_fwd(xl, il, long.reshape(-1, 512), 512, lens.reshape(-1), 3, 512, 0)
    ctc.nbest_log_likelihood(xl, long, None)                       # max_labels None: 511, the 512-label rows not live
    with pytest.raises(ValueError, match="blank"):
        ctc.expected_risk_loss(x, ids, lens, risk, blank=5)
    with pytest.raises(_lib.CfmError, match=r"\(-1\).*blank out of range"):
        ops.ctc_nbest_fwd(x, il, ids.reshape(-1, 4), 4, lens.reshape(-1), 3, 4, 5)
    with pytest.raises(_lib.CfmError, match=r"\(-2\).*bad shape"):      # max_labels beyond the rows' width
        ops.ctc_nbest_fwd(x, il, ids.reshape(-1, 4), 4, lens.reshape(-1), 3, 6, 0)
    with pytest.raises(RuntimeError):
        ctc.expected_risk_loss(x.cpu(), ids, lens, risk)
    with pytest.raises(RuntimeError):
        ctc.expected_risk_loss(x, ids.cpu(), lens, risk)
    with pytest.raises(RuntimeError):
        ctc.expected_risk_loss(x, ids, lens, risk.cpu())
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x, ids[:1], lens, risk)
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x, ids, lens[:, :2], risk)
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x, ids, lens, risk[:, :2])
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x, ids, [[5, 1, 1], [1, 1, 1]], risk)     # a host length beyond the rows' width
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x, ids, lens, risk, [8, 9])
    with pytest.raises(ValueError):
        ctc.expected_risk_loss(x[0], ids, lens, risk)
    with pytest.raises(TypeError):
        ctc.expected_risk_loss(x, ids.float(), lens, risk)


def _host_nbest(tokens, lens, scores):
    tokens, lens, scores = tokens.cpu(), lens.cpu(), scores.cpu()
    return [[None if scores[b, n] == -np.inf else tokens[b, n, :int(lens[b, n])].tolist()
             for n in range(tokens.shape[1])] for b in range(tokens.shape[0])]


def test_mwer_loss_equals_the_reference_on_the_devices_own_nbest():
    x, targets, il, tl = _mwer_inputs()
    xg = x.clone().requires_grad_()
    loss, ed, post = ctc.mwer_loss(xg, targets, il, tl, nbest=4, beam_size=8)
    loss.sum().backward()
    tokens, lens, scores = ctc.beam_search_decode(x, il, beam_size=8, nbest=4)
    hyps = _host_nbest(tokens, lens, scores)
    want_ed = ctc.edit_distance(tokens, targets, lens, tl)
    assert torch.equal(ed.distance, want_ed.distance) and ed.distance.shape == (3, 4)
    assert hyps[2][0] is not None and sum(h is not None for hb in hyps for h in hb) >= 6
    args = (x.cpu().numpy(), il.tolist(), hyps, ed.distance.cpu().tolist())
    ref, ref32 = nr.reference(*args), nr.reference(*args, dtype=torch.float32)
    assert np.abs(ref["grad"]).max() > 1e-3
    for key, got in (("post", post), ("loss", loss), ("grad", xg.grad)):
        got = got.detach().cpu().double().numpy()
        e, e32 = np.abs(got - ref[key]).max(), np.abs(ref32[key] - ref[key]).max()
        print(f"  mwer_loss {key}: err {e:.3g}  fp32 reference err {e32:.3g}")
        assert e <= 2 * e32 + 1e-7 * np.abs(ref[key]).max(), (key, e, e32)
    # time-major logits: the same numbers
    xt = x.transpose(0, 1).contiguous().requires_grad_()
    loss_t = ctc.mwer_loss(xt, targets, il, tl, nbest=4, beam_size=8, batch_first=False)[0]
    loss_t.sum().backward()
    assert torch.equal(loss_t, loss) and torch.equal(xt.grad.transpose(0, 1), xg.grad)


def test_one_step_along_the_gradient_raises_the_references_posterior():
    """The best hypothesis is [1, 2], the second best [1, 3] is the reference: a step along -grad moves posterior mass
    to the hypothesis with fewer word errors."""
    T, V = 6, 4
    x = torch.zeros(1, T, V)
    for t, v in enumerate((1, 1, 0, 2, 0, 0)):
        x[0, t, v] = 3.0
    x[0, 3, 3] = 2.5
    x = x.to(DEV).requires_grad_()
    targets = torch.tensor([[1, 3]], device=DEV)
    il, tl = torch.tensor([T], device=DEV), torch.tensor([2], device=DEV)
    loss, ed, post = ctc.mwer_loss(x, targets, il, tl, nbest=2, beam_size=4)
    tokens, lens, _ = ctc.beam_search_decode(x.detach(), il, beam_size=4, nbest=2)
    assert tokens[0, 0, :2].tolist() == [1, 2] and tokens[0, 1, :2].tolist() == [1, 3] and lens[0].tolist() == [2, 2]
    assert ed.distance[0].tolist() == [1, 0] and float(post[0, 0]) > float(post[0, 1]) > 0.05
    loss.sum().backward()
    stepped = (x - 1.0 * x.grad).detach()
    _, post2 = ctc.nbest_log_likelihood(stepped, tokens, lens, il)
    assert float(post2[0, 1]) > float(post[0, 1]) + 1e-3
    assert float(ctc.expected_risk_loss(stepped, tokens, lens, ed.distance.float(), il).loss) < float(loss)
