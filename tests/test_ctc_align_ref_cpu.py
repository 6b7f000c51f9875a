"""Pins the fp64 forced-alignment reference (tests/ctc_align_ref.py) and the inputs of tests/test_gpu_ctc_align.py:
viterbi against full enumeration, margin against the enumerated second best, the tie rule on uniform inputs written out
by hand, the infeasible rule, and -- what lets the GPU test demand path equality with no case left out -- every GPU
case decided by more than twice the fp32 roundoff bound."""
import itertools

import numpy as np
import pytest

from tests import ctc_align_ref as ar

V3, T6 = 3, 6


def _lp(seed, T, V):
    return ar.log_softmax(np.random.default_rng(seed).standard_normal((T, V)) * 2.0)


def _targets_upto3():
    out = [()]
    for L in (1, 2, 3):
        out += list(itertools.product(range(1, V3), repeat=L))
    return out


@pytest.mark.parametrize("T6", [6, 3])
def test_viterbi_equals_brute_force_for_every_short_target(T6):
    lp = _lp(0, T6, V3)
    n_inf = 0
    for tg in _targets_upto3():
        path, score = ar.viterbi(lp, tg)
        bpath, bscore, table = ar.brute_force(lp, tg, through=True)
        if not ar.feasible(T6, tg):
            n_inf += 1
            assert path is None and score == -np.inf and bpath is None and bscore == -np.inf
            continue
        assert abs(score - bscore) <= 1e-12, tg
        assert np.array_equal(path, bpath), tg                   # random inputs: no ties
        ext = ar.ext_labels(tg)
        assert abs(sum(lp[t, ext[s]] for t, s in enumerate(path)) - score) <= 1e-12
        # margin: the enumerated best alignment through any cell off the path
        th = ar.through_table(lp, tg)
        assert np.allclose(th, table, atol=1e-12, rtol=0)
        off = [bscore - max(table[t, s] for s in range(len(ext)) if s != path[t]) for t in range(T6) if len(ext) > 1]
        want = min(off) if off else np.inf
        m = ar.margin(lp, tg)
        assert m == want if np.isinf(want) else abs(m - want) <= 1e-12
    # T 6 fits every target of up to 3 labels; at T 3 the six with a repeat among 2 or 3 labels do not fit
    assert n_inf == (0 if T6 == 6 else 6)


def test_infeasible_rule():
    lp = _lp(1, 4, V3)
    for tg in [(1, 1, 1), (1, 1, 2, 2), (1, 2, 1, 2, 1), (2, 2, 1)]:
        assert ar.feasible(4, tg) == (4 >= len(tg) + ar.repeats(tg))
        path, score = ar.viterbi(lp, tg)
        bpath, bscore = ar.brute_force(lp, tg)
        assert (path is None) == (not ar.feasible(4, tg)) == (bpath is None)
        assert score == bscore or abs(score - bscore) <= 1e-12
    assert ar.viterbi(np.zeros((0, V3)), (1,)) == (None, -np.inf)
    path, score = ar.viterbi(np.zeros((0, V3)), ())
    assert len(path) == 0 and score == 0.0
    path, score = ar.viterbi(_lp(2, 3, V3), ())
    assert path.tolist() == [0, 0, 0]                             # no labels: all blank
    assert ar.repeats((1, 1, 2, 2, 2)) == 3


def test_tie_rule_on_uniform_logits_by_hand():
    """Every reachable state holds the same value, so the rule alone decides: the end prefers the final blank, and
    going back in time the path stays wherever the state was reachable a frame earlier, else comes from s-1, else
    skips.  T 6, target (1, 2): state 4 is first reachable at frame 2 (1 -> 3 -> 4), so 4 4 4 4 back to frame 2,
    frame 1 is state 3 (4's only predecessor there), and frame 0 is state 1 by the skip (0 -> 3 does not exist,
    2 is not reachable at frame 0).  Target (1, 1): no skip over the blank between equal labels, state 4 is first
    reachable at frame 3: 1 2 3 4 4 4."""
    lp = ar.log_softmax(np.zeros((6, 4)))
    path, score = ar.viterbi(lp, (1, 2))
    assert path.tolist() == [1, 3, 4, 4, 4, 4]
    assert abs(score - 6 * np.log(0.25)) <= 1e-12
    path, _ = ar.viterbi(lp, (1, 1))
    assert path.tolist() == [1, 2, 3, 4, 4, 4]
    path, _ = ar.viterbi(lp[:2], (1, 2))                          # tight: the last label ends the path
    assert path.tolist() == [1, 3]
    path, _ = ar.viterbi(lp[:1], (1,))
    assert path.tolist() == [1]


def test_plant_draws_valid_alignments():
    rng = np.random.default_rng(3)
    for tg, T in [((1, 2, 2, 3), 5), ((1, 2, 2, 3), 9), ((), 4), ((2,), 1), ((1, 1, 1), 5)]:
        for _ in range(20):
            p = ar.random_alignment(T, tg, rng)
            ext = ar.ext_labels(tg)
            assert len(p) == T
            assert np.array_equal(ar.states_from_labels(ext[p], tg), p)
    assert ar.random_alignment(4, (1, 1, 1), rng) is None


@pytest.mark.parametrize("name", list(ar.CASES))
def test_every_gpu_case_is_decided_by_more_than_roundoff(name):
    _, B, T, V, _, calls = ar.CASES[name]
    inputs = ar.case_inputs(name)
    assert len(inputs) == len(calls)
    n_feasible = 0
    for x, targets, ils in inputs:
        assert x.shape == (B, T, V) and x.dtype == np.float32
        for b in range(B):
            Tb = ils[b]
            assert all(0 < c < V for c in targets[b])
            lp = ar.log_softmax(x[b, :Tb])
            path, score = ar.viterbi(lp, targets[b])
            if path is None:
                assert not ar.feasible(Tb, targets[b])
                continue
            n_feasible += 1
            eps = ar.roundoff_eps(max(Tb, 1), abs(score))
            m = ar.margin(lp, targets[b])
            print(f"  {name} b {b}: T_b {Tb} L {len(targets[b])} score {score:.3f} margin {m:.3e} eps {eps:.3e}")
            assert m > 2 * eps, (name, b, m, eps)
    assert n_feasible >= 1
    if name == "ragged_empty_infeasible":
        x, targets, ils = inputs[0]
        assert [ar.feasible(t, g) for t, g in zip(ils, targets)] == [True, True, True, False]
    if name == "repeats_tight":
        x, targets, ils = inputs[0]
        assert [t - len(g) - ar.repeats(g) for t, g in zip(ils, targets)] == [1, 1, 10]
