"""Pins tests/ctc_nbest_ref.py, the fp64 reference of the n-best CTC likelihood and the expected risk over it: the
likelihood against brute force, the autograd gradient against the closed form without the softmax term, the
contract's exact zeros, and what each GPU case is there for."""
import itertools

import numpy as np
import pytest

from tests import ctc_nbest_ref as nr


def _logits(seed, T, V, scale=2.0):
    return np.random.default_rng(seed).standard_normal((T, V)) * scale


def test_ll_equals_brute_force():
    """Every hypothesis of 0-3 labels over V 3 (labels 1, 2; blank 0) at T 5, repeats and infeasible ones included."""
    x = _logits(0, 5, 3)
    lp = nr.log_softmax(x)
    hyps = [list(h) for L in range(4) for h in itertools.product((1, 2), repeat=L)]
    got = nr.expected_risk(x, hyps, [0.0] * len(hyps))["ll"]
    for h, g in zip(hyps, got):
        want = nr.brute_force_ll(lp, h, 0)
        assert np.isfinite(want) == nr.feasible(5, h)
        if np.isfinite(want):
            assert abs(g - want) <= 1e-12, (h, g, want)
            a, bt, em, ll = nr.alpha_beta(lp, h, 0)
            assert abs(ll - want) <= 1e-12
        else:
            assert g == -np.inf
    # blank != 0
    lp2 = nr.log_softmax(_logits(1, 4, 3))
    for h in ([0], [0, 1], [1, 1]):
        assert abs(nr.expected_risk(_logits(1, 4, 3), [h, []], [0, 1], blank=2)["ll"][0]
                   - nr.brute_force_ll(lp2, h, 2)) <= 1e-12


@pytest.mark.parametrize("seed,T,V,hyps", [
    (2, 6, 4, [[1, 2], [2, 2, 1], [], [3]]),
    (3, 9, 5, [[1, 1, 1], [4, 3, 4, 3], [2], None, [1, 2, 3, 4, 1, 2, 3, 4, 1, 2]]),
    (4, 5, 3, [[1, 1, 2], [2, 1]]),
])
def test_autograd_gradient_is_the_closed_form_without_softmax(seed, T, V, hyps):
    x = _logits(seed, T, V)
    risk = [float(k * k % 5) for k in range(len(hyps))]
    r = nr.expected_risk(x, hyps, risk)
    live = [h if h is not None else [] for h in hyps]
    closed = nr.grad_from_occ(x, live, r["c"])
    assert np.abs(r["grad"] - closed).max() <= 1e-12
    assert np.abs(r["grad"]).max() > 1e-3                               # (not vacuous)
    assert np.abs(r["grad"].sum(-1)).max() <= 1e-12                      # every row sums to 0 over the classes
    assert abs(r["c"].sum()) <= 1e-15 and abs(r["post"].sum() - 1) <= 1e-15
    used = {0} | {v for h, c in zip(live, r["c"]) if c != 0 for v in h}
    for v in range(V):
        if v not in used:
            assert (r["grad"][:, v] == 0).all() or np.abs(r["grad"][:, v]).max() <= 1e-15
    for n, h in enumerate(hyps):                                         # missing and infeasible: post 0
        if h is None or not nr.feasible(T, h):
            assert r["post"][n] == 0 and r["ll"][n] == -np.inf and r["c"][n] == 0
    # the occupancy of one hypothesis is a distribution over the classes at every frame
    occ = nr.occupancy(nr.log_softmax(x), live[0], 0)
    assert np.abs(occ.sum(-1) - 1).max() <= 1e-12


def test_equal_risks_one_live_and_none_live_give_zero():
    x = _logits(5, 7, 4)
    r = nr.expected_risk(x, [[1, 2], [3], [2, 2]], [2.0, 2.0, 2.0])
    assert r["loss"] == 0 and (r["grad"] == 0).all() and (r["c"] == 0).all() and abs(r["post"].sum() - 1) < 1e-15
    r = nr.expected_risk(x, [[1, 2], None, [1, 1, 1, 1, 2]], [0.0, 5.0, 9.0])   # the third needs 8 frames
    assert r["loss"] == 0 and (r["grad"] == 0).all() and r["post"].tolist() == [1.0, 0.0, 0.0]
    r = nr.expected_risk(x, [None, None], [0.0, 5.0])
    assert r["loss"] == 0 and (r["post"] == 0).all() and (r["ll"] == -np.inf).all()
    r = nr.expected_risk(x[:0], [[], [], [1]], [0.0, 4.0, 1.0])          # no frames: two empty hypotheses are live
    assert r["ll"].tolist() == [0.0, 0.0, -np.inf] and r["post"].tolist() == [0.5, 0.5, 0.0] and r["loss"] == 0.0
    r = nr.expected_risk(x, [[1, 2], [3, 3, 3], [2]], [0.0, 1.0, 5.0], max_labels=2)   # over max_labels: not live
    assert r["post"][1] == 0 and r["ll"][1] == -np.inf and r["loss"] != 0


def test_the_gpu_cases_exercise_what_their_names_say():
    C = nr.CASES
    for name, c in C.items():
        B, T, V = c["x"].shape
        ref = nr.reference(c["x"], c["ils"], c["hyps"], c["risks"], c["blank"], c["max_labels"])
        assert (np.isfinite(ref["ll"]).sum(1) >= 2).any(), name
        assert (ref["c"] != 0).any() and np.abs(ref["grad"]).max() > 1e-3, name      # (no degenerate posterior)
        print(f"  {name}: post {np.round(ref['post'], 4).tolist()}  max |grad| {np.abs(ref['grad']).max():.3g}")
        assert len({len(hb) for hb in c["hyps"]}) == 1, name
    lens = lambda name: [len(h) for hb in C[name]["hyps"] for h in hb if h is not None]
    assert C["ragged_T_0_and_1"]["ils"][2:] == [1, 0]
    assert C["V2"]["x"].shape[2] == 2 and C["V1024_N5"]["x"].shape[2] == 1024
    assert {len(c["hyps"][0]) for c in C.values()} >= {2, 5, 16}
    assert 0 in lens("S63_one_wave") and max(lens("S63_one_wave")) == 31 and C["S63_one_wave"]["max_labels"] == 31
    assert max(lens("S65_lds")) == 32 and C["S65_lds"]["max_labels"] == 32
    assert lens("wave_boundaries") == [63, 63, 64, 64, 100, 100, 129, 129]
    assert max(lens("L511_T520")) == 511 and C["L511_T520"]["ils"] == [520]
    assert np.isfinite(nr.reference(**C["L511_T520"])["ll"]).all()
    assert C["prefetch_block"]["ils"] == [15, 16, 17, 33]
    c = C["repeats_exact_and_infeasible"]
    h = c["hyps"][0][0]
    assert c["ils"] == [len(h) + nr.repeats(h), len(h) + nr.repeats(h) - 1] and nr.repeats(h) > 0
    ref = nr.reference(**c)
    assert np.isfinite(ref["ll"][0, 0]) and ref["ll"][1, 0] == -np.inf
    occ = nr.occupancy(nr.log_softmax(c["x"][0]), h, 0)
    assert np.allclose(np.sort(occ, -1)[:, -1], 1.0, atol=1e-12)        # one alignment: the occupancy is 0 / 1
    c = C["N16_missing_identical"]
    assert c["hyps"][0][0] == c["hyps"][0][1] and any(h is None for h in c["hyps"][0])
    ref = nr.reference(**c)
    assert ref["ll"][0, 0] == ref["ll"][0, 1] and (ref["post"][1, :13] == 0).all()
    c = C["over_max_labels"]
    ref = nr.reference(**c)
    assert ref["post"][0, 1] == 0 and ref["post"][1, 0] == 0 and c["hyps"][1][1] == c["hyps"][1][2]
