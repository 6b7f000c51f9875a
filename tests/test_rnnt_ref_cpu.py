"""tests/rnnt_ref.py pinned against itself: the alpha recursion against the sum over every path, the autograd gradient
against the closed form, and the cases of tests/test_gpu_rnnt.py against their names."""
import itertools
import re

import numpy as np
import pytest

from tests import rnnt_ref as rr

V3 = 3
TARGETS = [list(t) for n in range(4) for t in itertools.product((1, 2), repeat=n)]


def _x(T, U1, V, seed):
    return np.random.default_rng(seed).standard_normal((T, U1, V)) * 2


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_ll_equals_the_sum_over_every_path(T):
    for k, labels in enumerate(TARGETS):
        x = _x(T, len(labels) + 1, V3, 100 * T + k)
        want = rr.brute_force_ll(x, labels, 0)
        ll_a, _ = rr.ll_autograd(x, labels, 0)
        ll_c, _ = rr.closed_form_grad(x, labels, 0)
        assert abs(ll_a - want) <= 1e-12 and abs(ll_c - want) <= 1e-12, (T, labels)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_autograd_gradient_equals_the_closed_form(T):
    for k, labels in enumerate(TARGETS):
        x = _x(T, len(labels) + 1, V3, 200 * T + k)
        _, g_a = rr.ll_autograd(x, labels, 0)
        _, g_c = rr.closed_form_grad(x, labels, 0)
        assert np.abs(g_a - g_c).max() <= 1e-12, (T, labels)
        assert np.abs(g_c.sum(-1)).max() <= 1e-12          # every valid row sums to 0 over v


def test_alpha_side_ll_equals_beta_at_the_origin():
    for blank, labels in ((0, [1, 2, 2, 1]), (2, [0, 1, 3])):
        x = _x(5, len(labels) + 1, 4, 7 + blank)
        lp = rr.log_softmax_np(x, np.float64)
        alpha, beta, ll = rr.tables(*rr.emissions(lp, labels, blank))
        assert abs(ll - beta[0, 0]) <= 1e-12
        assert abs(ll - rr.brute_force_ll(x, labels, blank)) <= 1e-12
        # alpha + beta along any anti-diagonal sums to the total: every path crosses it once
        for d in range(1, 5 + len(labels) - 1):
            cells = [(t, d - t) for t in range(5) if 0 <= d - t <= len(labels)]
            assert abs(np.logaddexp.reduce([alpha[c] + beta[c] for c in cells]) - ll) <= 1e-12


def test_no_labels_is_the_sum_of_the_blanks():
    x = _x(6, 1, 5, 3)
    lp = rr.log_softmax_np(x, np.float64)
    for f in (rr.ll_autograd, rr.closed_form_grad):
        assert abs(f(x, [], 2)[0] - lp[:, 0, 2].sum()) <= 1e-12


def test_one_frame_is_the_single_path():
    x = _x(1, 4, 5, 4)
    lp = rr.log_softmax_np(x, np.float64)
    labels = [3, 1, 3]
    want = sum(lp[0, u, labels[u]] for u in range(3)) + lp[0, 3, 0]
    for f in (rr.ll_autograd, rr.closed_form_grad):
        assert abs(f(x, labels, 0)[0] - want) <= 1e-12


def test_batch_reference_zero_outside_and_without_frames():
    c = rr.CASES["ragged_T_0_and_1"]
    ref = rr.reference(**c)
    assert ref["ll"][0] == -np.inf and np.isfinite(ref["ll"][1:]).all()
    for b, (tb, ub) in enumerate(zip(c["ils"], c["tls"])):
        assert (ref["grad"][b, tb:] == 0).all() and (ref["grad"][b, :, ub + 1:] == 0).all()
        if tb:
            assert np.abs(ref["grad"][b, :tb, :ub + 1]).max() > 1e-3
    ref32 = rr.reference(**c, dtype=np.float32)
    assert 0 < np.abs(ref32["grad"] - ref["grad"]).max() < 1e-5


def test_cases_exercise_what_their_names_say():
    for name, c in rr.CASES.items():
        B, T, U1, V = c["x"].shape
        assert c["x"].dtype == np.float32 and c["targets"].shape == (B, U1 - 1)
        assert len(c["ils"]) == B and len(c["tls"]) == B
        assert all(0 <= t <= T for t in c["ils"]) and all(0 <= u <= U1 - 1 for u in c["tls"])
        assert not (c["targets"] == c["blank"]).any() and c["targets"].min(initial=V) >= 0
        assert c["targets"].max(initial=0) < V
        m = re.fullmatch(r"U1_(\d+)_T(\d+)_V(\d+)", name)
        if m:
            assert (U1, T, V) == tuple(int(g) for g in m.groups()), name
            assert B == 3 and c["ils"][-1] == T and max(c["tls"]) == U1 - 1      # the full lattice takes part
            assert T * U1 * V <= 160000
    shapes = [c["x"].shape for n, c in rr.CASES.items() if n.startswith("U1_")]
    assert {s[2] for s in shapes} == {1, 2, 9, 63, 64, 65, 256, 257, 1024}
    assert {s[1] for s in shapes} == {1, 2, 3, 17} and {s[3] for s in shapes} == {2, 5, 37, 1024}
    assert rr.CASES["U1_1024_T3_V2"]["x"].shape[1:] == (3, 1024, 2)
    c = rr.CASES["ragged_T_0_and_1"]
    assert 0 in c["ils"] and 1 in c["ils"] and c["x"].shape[1] in c["ils"]
    c = rr.CASES["ragged_U_0_and_Umax"]
    assert 0 in c["tls"] and c["x"].shape[2] - 1 in c["tls"] and len(set(c["tls"])) >= 3
    c = rr.CASES["repeated_labels"]
    assert all(any(a == b for a, b in zip(row[:-1], row[1:])) for row in c["targets"].tolist())
    assert rr.CASES["blank_not_0"]["blank"] == 3
    c = rr.CASES["blank_last"]
    assert c["blank"] == c["x"].shape[3] - 1
