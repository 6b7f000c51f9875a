"""CTC prefix beam search with an n-gram LM fused in on the device (csrc/ctc_beam.hip beam_search<true>,
ctc.beam_search_decode(..., lm=...), ASRNN.predict_beam, Runner with hp.decoder_lm) against the fp64 restatement of
tests/ctc_beam_lm_ref.py.

* replay: the device's back-pointer table is followed frame by frame in fp64 (ctc_beam_lm_ref.replay_lm): every slot
  a distinct member of the candidate set (stays, every entry times the token_beam best tokens of the frame), slots
  ordered, nothing better of that set left out, final scores and the n-best order after the </s> term equal, within
  eps = (8 T + 3) 2^-24 max(1, max |score|) (ctc_beam_lm_ref.ROUNDINGS_*; the reference reads the same fp32 table
  values, so table quantisation is not in eps).  Measured on the MI355X in profiles/beam_lm/replay_errors.txt;
* zero weights reproduce the no-LM decoder bit for bit; a constructed input on which the LM decides; free-running
  against full enumeration; determinism, graph replay and the likelihood bound at the label-pass shape; the Runner."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nn_conformer_for_speech_recognition_amd import ctc
from nn_conformer_for_speech_recognition_amd.lm import NGramLM
from tests import ctc_beam_lm_ref as lr
from tests import ctc_beam_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check_replay(x, out, trace, W, K, nbest, lm, alpha, beta, eos=True, lens=None, blank=0, pad=-1):
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
            fin = [((), alpha * lm.logp((lm.bos,), lm.eos) if eos else 0.0, 0)]
            eps = lr.roundoff_eps_lm(T, abs(fin[0][1]))
        else:
            fin, eps, viol = lr.replay_lm(x[b, :Tb], bp_parent[b], bp_token[b], W, K, lm, alpha, beta, eos, blank, pad,
                                          T_eps=T)
            worst = max(worst, viol["order"] / eps, viol["cut"] / eps)
        by_prefix = {p: sc for p, sc, _ in fin}
        ranked = sorted(sc for _, sc, _ in fin)[::-1]
        seen = set()
        for h in range(nbest):
            n = int(out_len[b, h])
            if h < len(fin):
                p = tuple(tokens[b, h, :n])
                assert p in by_prefix and p not in seen, (b, h, p)
                seen.add(p)
                d = float(score[b, h])
                # the score of this hypothesis, and the h-th best final score of the beam (the n-best order)
                assert abs(d - by_prefix[p]) <= eps, (b, h, d, by_prefix[p], eps)
                assert abs(d - ranked[h]) <= eps, (b, h, d, ranked[h], eps)
                worst = max(worst, abs(d - by_prefix[p]) / eps, abs(d - ranked[h]) / eps)
                assert blank not in p and (pad < 0 or pad not in p)
            else:
                assert n == 0 and score[b, h] == -np.inf
            assert (tokens[b, h, n:] == -1).all()
            if h and np.isfinite(score[b, h]):
                assert score[b, h - 1] >= score[b, h]
    print(f"  B {B} T {T} V {V} W {W} K {K} nbest {nbest} alpha {alpha} beta {beta} eos {eos}: "
          f"worst (violation or score error) / eps = {worst:.4f}")


def _sparse_lm(seed, V, **kw):
    return lr.random_lm(seed, V, n_bi=400, n_tri=800, **kw)


CASES = {
    # name: (logits seed, B, T, V, W, K, nbest, scale, lens, alpha, beta, lm)
    "ragged_and_empty": (11, 3, 33, 5, 4, 4, 3, 2.0, [33, 1, 0], 0.8, 1.0, lambda: lr.random_lm(1, 5)),
    "mid_size": (12, 2, 64, 40, 16, 8, 4, 3.0, None, 0.6, 0.3, lambda: _sparse_lm(2, 40)),
    "single_token": (16, 2, 24, 2, 4, 1, 4, 2.0, None, 0.9, 0.4, lambda: lr.random_lm(3, 2)),
    "width_1": (17, 2, 24, 40, 1, 1, 1, 3.0, None, 0.7, 0.2, lambda: _sparse_lm(4, 40)),
    "candidate_limit": (20, 1, 24, 40, 32, 31, 8, 2.0, None, 0.5, 0.5, lambda: _sparse_lm(6, 40)),
}


def _run(x, lm, W, K, nbest, alpha, beta, lens=None, **kw):
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    *out, trace = ctc.beam_search_decode(x, ln, beam_size=W, nbest=nbest, return_trace=True, lm=lm, lm_weight=alpha,
                                         word_bonus=beta, token_beam=K, **kw)
    return out, trace


@pytest.mark.parametrize("name", list(CASES))
def test_replay(name):
    seed, B, T, V, W, K, nbest, scale, lens, alpha, beta, make_lm = CASES[name]
    x = br.make_logits(seed, B, T, V, scale)
    lm = make_lm()
    out, trace = _run(torch.from_numpy(x).to(DEV), lm, W, K, nbest, alpha, beta, lens)
    _check_replay(x, out, trace, W, K, nbest, lm, alpha, beta, True, lens)


def test_replay_without_the_sentence_end_term():
    seed, B, T, V, W, K, nbest, scale, lens, alpha, beta, make_lm = CASES["mid_size"]
    x = br.make_logits(seed, B, T, V, scale)
    lm = make_lm()
    out, trace = _run(torch.from_numpy(x).to(DEV), lm, W, K, nbest, alpha, beta, lens, lm_eos=False)
    _check_replay(x, out, trace, W, K, nbest, lm, alpha, beta, False, lens)


def test_replay_sparse_trigram():
    s = lr.SPARSE
    x = lr.sparse_logits()
    lm = lr.random_lm(**s["lm"])
    out, trace = _run(torch.from_numpy(x).to(DEV), lm, s["W"], s["K"], s["nbest"], s["alpha"], s["beta"])
    _check_replay(x, out, trace, s["W"], s["K"], s["nbest"], lm, s["alpha"], s["beta"])


def test_replay_pad_is_never_emitted():
    x = br.make_logits(18, 2, 24, 8, 3.0)
    x[..., 1] += 4.0                                          # the pad column would win most frames
    lm = lr.random_lm(7, 8, pad=1)
    out, trace = _run(torch.from_numpy(x).to(DEV), lm, 8, 6, 8, 0.8, 0.3, pad=1)
    assert not (out[0] == 1).any() and not (trace[1] == 1).any()
    _check_replay(x, out, trace, 8, 6, 8, lm, 0.8, 0.3, pad=1)


def test_replay_time_major_and_strided_rows():
    x = br.make_logits(19, 3, 24, 12, 3.0)
    lens = [24, 17, 5]
    lm = lr.random_lm(8, 12, n_bi=60, n_tri=200)
    tm = torch.from_numpy(x).to(DEV).transpose(0, 1).contiguous()                       # (T, B, V)
    out, trace = _run(tm, lm, 6, 5, 2, 0.7, 0.1, lens, batch_first=False)
    _check_replay(x, out, trace, 6, 5, 2, lm, 0.7, 0.1, lens=lens)
    wide = torch.full((3, 24, 12 + 7), 50.0, device=DEV)                                # a row stride wider than V
    wide[..., :12] = torch.from_numpy(x).to(DEV)
    view = wide[..., :12]
    assert view.stride(-1) == 1 and view.stride(1) == 19
    out2, trace2 = _run(view, lm, 6, 5, 2, 0.7, 0.1, lens)
    _check_replay(x, out2, trace2, 6, 5, 2, lm, 0.7, 0.1, lens=lens)
    for a, c in zip(out, out2):
        assert torch.equal(a, c)


@pytest.mark.parametrize("name", ["w16", "ragged_and_empty"])
def test_zero_weights_reproduce_the_plain_decoder(name):
    from tests.test_gpu_ctc_beam import CASES as PLAIN
    seed, B, T, V, W, nbest, scale, lens = PLAIN[name]
    x = torch.from_numpy(br.make_logits(seed, B, T, V, scale)).to(DEV)
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    lm = lr.random_lm(9, V) if V <= 8 else _sparse_lm(9, V)
    *want, wtrace = ctc.beam_search_decode(x, ln, beam_size=W, nbest=nbest, return_trace=True)
    *got, gtrace = ctc.beam_search_decode(x, ln, beam_size=W, nbest=nbest, return_trace=True, lm=lm, lm_weight=0.0,
                                          word_bonus=0.0, token_beam=W + 1, lm_eos=False)
    for a, c in zip(want, got):                               # tokens, lengths, scores (bit-equal)
        assert a.dtype == c.dtype and torch.equal(a, c)
    for b in range(B):                                        # the back-pointers of the valid frames
        Tb = T if lens is None else lens[b]
        for a, c in zip(wtrace, gtrace):
            assert torch.equal(a[b, :Tb], c[b, :Tb])


def test_the_lm_decides():
    """Token 1, then a one-frame segment on which 2 leads 3 acoustically by 0.6; the bigram prefers (1, 3) to (1, 2)
    by 3.9, more than the acoustic margin + 1e-3: with the LM the decode says 1 3, without it 1 2."""
    V, T = 4, 8
    x = np.full((1, T, V), -4.0, np.float32)
    for t, c in enumerate([0, 1, 1, 0, 2, 0, 0, 0]):
        x[0, t, c] = 6.0 if c != 2 else 5.0
    x[0, 4, 3] = 4.4
    g = {(1,): (-1.5, -0.2), (2,): (-1.5, -0.2), (3,): (-1.5, -0.2), (V,): (-200.0, -0.1), (V + 1,): (-1.5, 0.0),
         (1, 3): (-0.1, 0.0), (1, 2): (-4.0, 0.0)}
    lm = NGramLM(g, V, 0, -1, 2)
    assert lm.logp((1,), 3) - lm.logp((1,), 2) > 0.6 + 1e-3
    plain_ref, _ = br.full_search(br.log_softmax(x[0]), 4)
    fused_ref, _ = lr.full_search_lm(x[0], 4, lm, 1.0, 0.0)
    assert plain_ref[0][0] == (1, 2) and fused_ref[0][0] == (1, 3)
    xd = torch.from_numpy(x).to(DEV)
    tok, n, sc = ctc.beam_search_decode(xd, beam_size=4)
    assert tok[0, 0, :int(n[0, 0])].tolist() == [1, 2]
    assert abs(float(sc[0, 0]) - plain_ref[0][1]) <= br.roundoff_eps(T, abs(plain_ref[0][1]))
    tok, n, sc = ctc.beam_search_decode(xd, beam_size=4, lm=lm, lm_weight=1.0)
    assert tok[0, 0, :int(n[0, 0])].tolist() == [1, 3]
    assert abs(float(sc[0, 0]) - fused_ref[0][1]) <= lr.roundoff_eps_lm(T, abs(fused_ref[0][1]))


def test_free_running_equals_full_enumeration():
    e = lr.E2E
    x = br.make_logits(e["seed"], e["B"], e["T"], e["V"], e["scale"])
    lm = lr.random_lm(e["lm_seed"], e["V"])
    for alpha, beta in e["weights"]:
        tokens, out_len, score = (o.cpu().numpy() for o in ctc.beam_search_decode(
            torch.from_numpy(x).to(DEV), beam_size=e["W"], nbest=e["nbest"], lm=lm, lm_weight=alpha, word_bonus=beta,
            token_beam=e["K"]))
        skipped = 0
        for b in range(e["B"]):
            hyps, gap = lr.full_search_lm(x[b], e["W"], lm, alpha, beta, nbest=e["nbest"])
            if gap <= e["min_gap"]:
                skipped += 1
                continue
            for h, (p, sc) in enumerate(hyps):
                n = int(out_len[b, h])
                assert tuple(tokens[b, h, :n]) == p, (alpha, beta, b, h)
                assert abs(float(score[b, h]) - sc) <= lr.roundoff_eps_lm(e["T"], abs(sc))
        print(f"  free-running alpha {alpha} beta {beta}: {skipped} of {e['B']} utterances skipped "
              f"(reference gap <= {e['min_gap']})")
        assert skipped <= 8


def test_label_pass_shape_likelihood_bound_determinism_and_capture():
    """score <= CTC log-likelihood + alpha (sum of lm + lm(</s>)) + beta |l| + eps for each hypothesis (the beam sums
    a subset of its alignments); two runs and two replays of a captured graph are bit-identical."""
    B, T, V, W, alpha, beta = 4, 373, 1024, 16, 0.5, 0.2
    s = lr.SPARSE
    x = br.make_logits(5, B, T, V, 4.0)
    x[..., 1:1 + s["hot"]] += np.float32(s["bump"])
    lm = lr.random_lm(**s["lm"])
    xd = torch.from_numpy(x).to(DEV)
    kw = dict(beam_size=W, nbest=2, lm=lm, lm_weight=alpha, word_bonus=beta)
    tokens, out_len, score = ctc.beam_search_decode(xd, **kw)
    lp = torch.from_numpy(x).double().log_softmax(-1).transpose(0, 1)                   # (T, B, V) fp64, CPU
    for h in range(2):
        tok, n = tokens[:, h].cpu().long().clamp(min=0), out_len[:, h].cpu().long()
        ll = -F.ctc_loss(lp, tok, torch.full((B,), T, dtype=torch.long), n, blank=0, reduction="none")
        for b in range(B):
            p = tuple(tok[b, :int(n[b])].tolist())
            lms = sum(lm.logp(lm.context(p[:i]), c) for i, c in enumerate(p)) + lm.logp(lm.context(p), lm.eos)
            bound = float(ll[b]) + alpha * lms + beta * len(p)
            sc = float(score[b, h])
            eps = lr.roundoff_eps_lm(T, abs(sc))
            print(f"  b {b} h {h}: score {sc:.4f}  bound {bound:.4f}  |l| {len(p)}  eps {eps:.4f}")
            assert len(p) > 0 and sc <= bound + eps
    again = ctc.beam_search_decode(xd, **kw)
    for a, c in zip((tokens, out_len, score), again):
        assert torch.equal(a, c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc.beam_search_decode(xd, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ctc.beam_search_decode(xd, **kw)
    for _ in range(2):
        for o in static:
            o.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for a, c in zip((tokens, out_len, score), static):
            assert torch.equal(a, c)


def test_runner_labels_with_the_decoder_lm():
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
    assert hp.decoder_lm is None and hp.lm_weight == 0.0 and hp.word_bonus == 0.0 and hp.token_beam == 0
    greedy = runner.generate_labels(ds)
    hp.set_beam_size(4)
    beam = runner.generate_labels(ds)
    lm = NGramLM.from_dataset(ds, "train")
    assert lm.V == len(vocab) and lm.order == 3 and lm.has_eos
    hp.set_decoder_lm(lm, 0.5)
    want = []
    with torch.no_grad():
        for i in range(2):
            batch = ds.get_batch(i, "pretrain")["input"]
            logits, lens = runner.model(batch["mels"], batch["tau"])
            bt, bn, _ = ctc.beam_search_decode(logits, lens, beam_size=4, blank=vocab.blank_idx, pad=vocab.pad_idx,
                                               lm=lm, lm_weight=0.5)
            want += vocab.decode(bt[:, 0], bn[:, 0])
            pt, pn = runner.model.predict_beam(logits, lens, beam_size=4, pad=vocab.pad_idx, lm=lm, lm_weight=0.5)
            assert torch.equal(pt, bt[:, 0]) and torch.equal(pn, bn[:, 0])
    assert runner.generate_labels(ds) == want
    loss, metric = runner.test(ds, "validation")
    assert np.isfinite(loss) and metric >= 0.0
    hp.set_decoder_lm(None)
    assert runner.generate_labels(ds) == beam
    hp.set_beam_size(0)
    assert runner.generate_labels(ds) == greedy


def test_argument_errors():
    x = torch.zeros(2, 5, 6, device=DEV)
    lm = lr.random_lm(1, 6)
    with pytest.raises(ValueError):                           # V mismatch
        ctc.beam_search_decode(x, beam_size=4, lm=lr.random_lm(1, 5), lm_weight=0.5)
    with pytest.raises(ValueError):                           # blank mismatch
        ctc.beam_search_decode(x, beam_size=4, blank=2, lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError):                           # pad mismatch
        ctc.beam_search_decode(x, beam_size=4, pad=1, lm=lm, lm_weight=0.5)
    big = torch.zeros(1, 4, 64, device=DEV)
    with pytest.raises(ValueError):                           # 32 + 32 * 32 > 1024
        ctc.beam_search_decode(big, beam_size=32, lm=_sparse_lm(1, 64), lm_weight=0.5, token_beam=32)
    for kw in (dict(lm_weight=0.5), dict(word_bonus=0.1), dict(token_beam=4), dict(lm_eos=False)):
        with pytest.raises(ValueError):                       # LM arguments without an LM
            ctc.beam_search_decode(x, beam_size=4, **kw)
    assert ctc.default_token_beam(16, 1023) == 17 and ctc.default_token_beam(128, 1023) == 7
    assert ctc.default_token_beam(4, 3) == 3
