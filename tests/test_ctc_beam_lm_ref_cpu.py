"""The yardstick of the LM-fused CTC beam search (tests/ctc_beam_lm_ref.py) pinned on the CPU.

* zero weights, no </s> term: the no-LM restatement exactly;
* brute force: where the beam holds every prefix the best hypothesis maximises
  ctc_loglik(l) + alpha (sum of lm + lm(</s>)) + beta |l| over all labellings;
* token_beam >= #tokens: the grid search is the full search;
* the free-running cases of tests/test_gpu_ctc_beam_lm.py are decidable, and its sparse case walks every back-off
  path."""
import itertools

import numpy as np
import pytest

from tests import ctc_beam_lm_ref as lr
from tests import ctc_beam_ref as br


def _x(seed, T, V, scale=2.0):
    return br.make_logits(seed, 1, T, V, scale)[0]


@pytest.mark.parametrize("T,V,W", [(30, 4, 3), (30, 5, 6), (24, 12, 8)])
def test_zero_weights_equal_the_plain_search(T, V, W):
    lm = lr.random_lm(2, V)
    for seed in range(8):
        x = _x(2000 + seed, T, V)
        lp = br.log_softmax(x)
        want, gap = br.full_search(lp, W, nbest=W)
        got, gap_lm = lr.full_search_lm(x, W, lm, 0.0, 0.0, eos=False, nbest=W)
        assert got == want and gap_lm == gap
        grid, _ = lr.grid_search_lm(x, W, W + 1, lm, 0.0, 0.0, eos=False, nbest=W)
        assert grid == br.pruned_search(lp, W, nbest=W)


def test_full_search_is_brute_force_when_nothing_is_pruned():
    T, V = 5, 3
    labels = [s for n in range(T + 1) for s in itertools.product(range(1, V), repeat=n)]
    lm = lr.random_lm(3, V)
    assert lm.order == 3
    for seed, (alpha, beta) in zip(range(6), [(0.5, 0.0), (0.8, 1.0), (1.5, -0.5)] * 2):
        x = _x(seed, T, V)
        lp = br.log_softmax(x)

        def fused(s):
            lms = sum(lm.logp(lm.context(s[:i]), c) for i, c in enumerate(s)) + lm.logp(lm.context(s), lm.eos)
            return br.ctc_loglik(lp, s) + alpha * lms + beta * len(s)

        tot = {s: fused(s) for s in labels}
        best = max(tot, key=tot.get)
        hyps, _ = lr.full_search_lm(x, len(labels) + 1, lm, alpha, beta, eos=True, nbest=len(labels))
        assert hyps[0][0] == best and abs(hyps[0][1] - tot[best]) < 1e-9
        for p, sc in hyps:
            assert abs(sc - tot[p]) < 1e-9, (p, sc, tot[p])


@pytest.mark.parametrize("T,V,W", [(30, 4, 3), (30, 4, 6), (30, 5, 2), (24, 12, 8)])
def test_full_grid_equals_full_search(T, V, W):
    lm = lr.random_lm(4, V)
    for seed in range(6):
        x = _x(3000 + seed, T, V)
        full = lr.full_search_lm(x, W, lm, 0.9, 0.3, nbest=W)
        assert lr.grid_search_lm(x, W, V - 1, lm, 0.9, 0.3, nbest=W) == full
        assert lr.grid_search_lm(x, W, V + 5, lm, 0.9, 0.3, nbest=W) == full


def test_pad_is_never_scored_or_emitted():
    lm = lr.random_lm(5, 6, pad=2)
    x = _x(7, 20, 6)
    x[:, 2] += 3.0
    hyps, _ = lr.full_search_lm(x, 4, lm, 0.8, 0.2, blank=0, pad=2, nbest=4)
    assert hyps and all(2 not in p and 0 not in p for p, _ in hyps)
    assert 2 not in lr.ranked_tokens(x[0], 5, 0, 2) and len(lr.ranked_tokens(x[0], 9, 0, 2)) == 4


def test_end_to_end_cases_are_decidable():
    """The free-running comparison skips utterances whose smallest reference gap is <= 1e-3: at most 4 of 32 per
    weight setting, on the fp64 reference alone."""
    e = lr.E2E
    lm = lr.random_lm(e["lm_seed"], e["V"])
    x = br.make_logits(e["seed"], e["B"], e["T"], e["V"], e["scale"])
    for alpha, beta in e["weights"]:
        res = [lr.full_search_lm(x[b], e["W"], lm, alpha, beta, nbest=e["nbest"]) for b in range(e["B"])]
        skipped = sum(gap <= e["min_gap"] for _, gap in res)
        print(f"  alpha {alpha} beta {beta}: {skipped} of {e['B']} skipped")
        assert skipped <= 4, (alpha, beta, skipped)
        worst = max(abs(sc) for hyps, _ in res for _, sc in hyps)
        assert 2 * lr.roundoff_eps_lm(e["T"], worst) <= e["min_gap"]     # the skip threshold is >= 2 eps here


def test_sparse_case_takes_every_back_off_path():
    s = lr.SPARSE
    lm = lr.random_lm(**s["lm"])
    x = lr.sparse_logits()
    trace = {}
    for b in range(s["B"]):
        hyps, _ = lr.grid_search_lm(x[b], s["W"], s["K"], lm, s["alpha"], s["beta"], nbest=s["nbest"], trace=trace)
        assert hyps and all(len(p) > 2 for p, _ in hyps[:1])
    print("  back-off paths of the sparse case:", dict(sorted(trace.items())))
    for path in ("tri", "bi", "uni", "backoff_seen", "backoff_unseen"):
        assert trace.get(path, 0) >= 1, (path, trace)
