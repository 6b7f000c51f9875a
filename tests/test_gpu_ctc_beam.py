"""CTC prefix beam search on the device (csrc/ctc_beam.hip, ctc.beam_search_decode, ASRNN.predict_beam, Runner with
hp.beam_size > 0) against the fp64 restatement of tests/ctc_beam_ref.py.

* replay: the device's back-pointer table is followed frame by frame in fp64 (ctc_beam_ref.replay): every slot a
  distinct candidate, slots ordered, nothing better left out, within eps = 4 T 2^-24 max(1, max |score|) (four fp32
  roundings per frame on a score path); tokens, lengths and scores then equal the replayed ones (scores within eps).
  Exact without skipping near-ties.  Measured on the MI355X (max score error / eps per case) in DESIGN.md §1;
* free-running: hypotheses == full enumeration wherever the reference's smallest gap exceeds 1e-3;
* peaked inputs == collapsed greedy decode; the label-pass shape against the CTC likelihood, run-to-run and graph
  replay bit-identity; the Runner's label pass with hp.beam_size."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nn_conformer_for_speech_recognition_amd import ctc
from tests import ctc_beam_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check_replay(x, out, trace, W, nbest, lens=None, blank=0, pad=-1):
    """x (B, T, V) fp32 numpy (the logical logits); out = (tokens, out_len, score) of the device."""
    B, T, V = x.shape
    tokens, out_len, score = (o.cpu().numpy() for o in out)
    bp_parent, bp_token = (o.cpu().numpy() for o in trace)
    assert tokens.shape == (B, nbest, T) and out_len.shape == (B, nbest) and score.shape == (B, nbest)
    assert bp_parent.shape == (B, T, W) and bp_token.shape == (B, T, W)
    worst = 0.0
    for b in range(B):
        Tb = T if lens is None else min(max(int(lens[b]), 0), T)
        if Tb == 0:
            hyps, eps = [((), 0.0)], br.roundoff_eps(T, 1.0)
        else:
            hyps, eps, viol = br.replay(br.log_softmax(x[b, :Tb]), bp_parent[b], bp_token[b], W, blank, pad, T_eps=T)
            worst = max(worst, viol["order"] / eps, viol["cut"] / eps)
        for h in range(nbest):
            n = int(out_len[b, h])
            if h < len(hyps):
                p, sc = hyps[h]
                assert tuple(tokens[b, h, :n]) == p, (b, h)
                assert abs(float(score[b, h]) - sc) <= eps, (b, h, float(score[b, h]), sc, eps)
                worst = max(worst, abs(float(score[b, h]) - sc) / eps)
                assert blank not in p and (pad < 0 or pad not in p)
            else:
                assert n == 0 and score[b, h] == -np.inf
            assert (tokens[b, h, n:] == -1).all()
            if h and np.isfinite(score[b, h]):
                assert score[b, h - 1] >= score[b, h] - eps            # n-best order
    print(f"  B {B} T {T} V {V} W {W} nbest {nbest}: worst (violation or score error) / eps = {worst:.4f}")


CASES = {
    # name: (seed, B, T, V, W, nbest, scale, lens)
    "ragged_and_empty": (11, 3, 33, 5, 4, 3, 2.0, [33, 1, 0]),
    "w16": (12, 2, 64, 40, 16, 4, 3.0, None),
    "more_slots_than_tokens": (13, 2, 24, 40, 64, 64, 4.0, None),
    "w128": (14, 1, 24, 300, 128, 100, 2.0, None),
    "v1024": (15, 2, 24, 1024, 32, 3, 3.0, None),
    "v2": (16, 2, 24, 2, 4, 4, 2.0, None),
    "w1": (17, 2, 24, 40, 1, 1, 3.0, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_replay(name):
    seed, B, T, V, W, nbest, scale, lens = CASES[name]
    x = br.make_logits(seed, B, T, V, scale)
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    *out, trace = ctc.beam_search_decode(torch.from_numpy(x).to(DEV), ln, beam_size=W, nbest=nbest,
                                         return_trace=True)
    _check_replay(x, out, trace, W, nbest, lens)


def test_replay_pad_is_never_emitted():
    x = br.make_logits(18, 2, 24, 8, 3.0)
    x[..., 1] += 4.0                                          # the pad column would win most frames
    *out, trace = ctc.beam_search_decode(torch.from_numpy(x).to(DEV), beam_size=8, pad=1, nbest=8, return_trace=True)
    assert not (out[0] == 1).any() and not (trace[1] == 1).any()
    _check_replay(x, out, trace, 8, 8, pad=1)


def test_replay_time_major_and_strided_rows():
    x = br.make_logits(19, 3, 24, 12, 3.0)
    lens = [24, 17, 5]
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tm = torch.from_numpy(x).to(DEV).transpose(0, 1).contiguous()                       # (T, B, V)
    *out, trace = ctc.beam_search_decode(tm, ln, beam_size=6, nbest=2, batch_first=False, return_trace=True)
    _check_replay(x, out, trace, 6, 2, lens)
    wide = torch.full((3, 24, 12 + 7), 50.0, device=DEV)                                # a row stride wider than V
    wide[..., :12] = torch.from_numpy(x).to(DEV)
    view = wide[..., :12]
    assert view.stride(-1) == 1 and view.stride(1) == 19
    *out2, trace2 = ctc.beam_search_decode(view, ln, beam_size=6, nbest=2, return_trace=True)
    _check_replay(x, out2, trace2, 6, 2, lens)
    for a, c in zip(out, out2):
        assert torch.equal(a, c)


def test_free_running_equals_full_enumeration():
    e = br.E2E
    x = br.make_logits(e["seed"], e["B"], e["T"], e["V"], e["scale"])
    tokens, out_len, score = (o.cpu().numpy() for o in
                              ctc.beam_search_decode(torch.from_numpy(x).to(DEV), beam_size=e["W"], nbest=e["nbest"]))
    skipped = 0
    for b in range(e["B"]):
        hyps, gap = br.full_search(br.log_softmax(x[b]), e["W"], nbest=e["nbest"])
        if gap <= e["min_gap"]:
            skipped += 1
            continue
        for h, (p, sc) in enumerate(hyps):
            n = int(out_len[b, h])
            assert tuple(tokens[b, h, :n]) == p, (b, h)
            assert abs(float(score[b, h]) - sc) <= br.roundoff_eps(e["T"], abs(sc))
    print(f"  free-running: {skipped} of {e['B']} utterances skipped (reference gap <= {e['min_gap']})")
    assert skipped <= 8


def test_peaked_inputs_equal_collapsed_greedy():
    path = [0, 3, 3, 0, 3, 2, 2, 2, 0, 0, 1, 4, 4, 0, 4, 4, 1, 1, 2, 0, 5, 5, 0, 0, 5, 3, 0]
    V = 6
    x = torch.zeros(2, len(path), V)
    x[0, torch.arange(len(path)), torch.tensor(path)] = 20.0
    rev = path[::-1]
    x[1, torch.arange(len(path)), torch.tensor(rev)] = 20.0
    x = x.to(DEV)
    _, want, want_n = ctc.greedy_decode(x, blank=0, collapse=True)
    tokens, out_len, score = ctc.beam_search_decode(x, beam_size=4)
    assert torch.equal(out_len[:, 0], want_n)
    assert torch.equal(tokens[:, 0], want)
    assert want_n.tolist() == [11, 11]                       # 3 3 2 1 4 4 1 2 5 5 3: repeats kept only across a blank
    assert score.abs().max().item() < 1e-3


def test_label_pass_shape_likelihood_bounds_and_determinism():
    """score <= log-likelihood of the hypothesis + eps (the beam sums a subset of its alignments) and, for the best
    hypothesis, score >= log-likelihood of the W 1 result's hypothesis - eps.  The lower bound is a property of the
    search as well as of the arithmetic (how much alignment mass a width-16 beam keeps), so the logit scale is chosen
    on the fp64 reference alone: at 4 * randn full enumeration is within 0.013 of that likelihood on all four
    utterances (eps 0.032); at 3 * randn the fp64 reference itself misses it on one (0.049 against eps 0.048)."""
    B, T, V, W = 4, 373, 1024, 16
    x = br.make_logits(5, B, T, V, 4.0)
    xd = torch.from_numpy(x).to(DEV)
    tokens, out_len, score = ctc.beam_search_decode(xd, beam_size=W, nbest=2)
    t1, n1, s1 = ctc.beam_search_decode(xd, beam_size=1)
    lp = torch.from_numpy(x).double().log_softmax(-1).transpose(0, 1)                   # (T, B, V) fp64, CPU

    def loglik(tok, n):
        """-ctc_loss(reduction='none') of hypotheses tok (B, T) / n (B,) on the same logits (torch, fp64, CPU)."""
        tok, n = tok.cpu().long().clamp(min=0), n.cpu().long()
        return -F.ctc_loss(lp, tok, torch.full((B,), T, dtype=torch.long), n, blank=0, reduction="none")

    ll_w1 = loglik(t1[:, 0], n1[:, 0])
    for h in range(2):
        ll = loglik(tokens[:, h], out_len[:, h])
        for b in range(B):
            sc = float(score[b, h])
            eps = br.roundoff_eps(T, abs(sc))
            print(f"  b {b} h {h}: score {sc:.4f}  loglik {float(ll[b]):.4f}  W1 loglik {float(ll_w1[b]):.4f}  "
                  f"eps {eps:.4f}")
            assert sc <= float(ll[b]) + eps                  # the beam sums a subset of the hypothesis's alignments
            if h == 0:
                assert sc >= float(ll_w1[b]) - eps
    again = ctc.beam_search_decode(xd, beam_size=W, nbest=2)
    for a, c in zip((tokens, out_len, score), again):
        assert torch.equal(a, c)
    # a captured graph replays to the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc.beam_search_decode(xd, beam_size=W, nbest=2)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ctc.beam_search_decode(xd, beam_size=W, nbest=2)
    for _ in range(2):
        for o in static:
            o.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for a, c in zip((tokens, out_len, score), static):
            assert torch.equal(a, c)


def test_runner_labels_with_and_without_beam():
    from nn_conformer_for_speech_recognition_amd.lib.standard.asrnn import ASRNN
    from nn_conformer_for_speech_recognition_amd.lib.standard.runner import Runner
    from tests.test_gpu_nst import _dataset, _hp, _vocab
    vocab = _vocab()
    hp = _hp(vocab, 1, 144, 4, 576, 15, "bf16", 4)
    ds = _dataset(hp, vocab, 2, 6, 201, 21)
    torch.manual_seed(4)
    m = ASRNN(hp)
    with torch.no_grad():
        m.final_fc.weight.mul_(8.0)
    runner = Runner(m, hp)
    assert hp.beam_size == 0
    today = runner.generate_labels(ds)
    want_greedy, want_beam = [], []
    with torch.no_grad():
        for i in range(2):
            batch = ds.get_batch(i, "pretrain")["input"]
            logits, lens = runner.model(batch["mels"], batch["tau"])
            _, toks, cnt = ctc.greedy_decode(logits, None, blank=vocab.blank_idx, pad=vocab.pad_idx, collapse=False)
            want_greedy += vocab.decode(toks, cnt)
            bt, bn, _ = ctc.beam_search_decode(logits, lens, beam_size=4, blank=vocab.blank_idx, pad=vocab.pad_idx)
            want_beam += vocab.decode(bt[:, 0], bn[:, 0])
            pt, pn = runner.model.predict_beam(logits, lens, beam_size=4, pad=vocab.pad_idx)
            assert torch.equal(pt, bt[:, 0]) and torch.equal(pn, bn[:, 0])
    assert today == want_greedy
    hp.set_beam_size(4)
    assert runner.generate_labels(ds) == want_beam
    loss, metric = runner.test(ds, "validation")
    assert np.isfinite(loss) and metric >= 0.0
    hp.set_beam_size(0)
    assert runner.generate_labels(ds) == today
