"""fp64 restatement of CTC forced alignment (test infrastructure; csrc/ctc_align.hip, ctc.forced_align), never calling
the library.

States of a target l_1 .. l_L: blank, l_1, blank, l_2, ..., blank (S = 2 L + 1).  Over log-probabilities lp (T, V):
  v[0, 0] = lp[0, blank], v[0, 1] = lp[0, l_1], the rest -inf;
  v[t, s] = lp[t, ext(s)] + max(v[t-1, s], v[t-1, s-1], v[t-1, s-2] if s is odd and ext(s) != ext(s-2)).
Tie rule (part of the contract): among equal predecessors stay wins, then s-1, then s-2 (a later candidate must be
strictly better); at the last frame S-1 wins a tie against S-2.  A target is infeasible when T < L + (number of
adjacent equal labels).

* viterbi       the recursion with back-pointers and that tie rule;
* brute_force   every one of the V^T labellings that collapses to the target, with its state path;
* margin        how far the best alignment is from being undecided: forward and backward max-plus tables give
                through[t, s], the best alignment through each cell; the smallest gap over the frames between the best
                and the runner-up state.  A device path can differ from the reference's only if margin <= 2 eps (fp32
                addition is monotone, so the device's recursion returns the path of largest fp32-evaluated score; it
                and the reference's path are each within eps of their fp64 scores);
* plant         raises the logits along a random valid alignment so that the optimum is decided by far more than
                roundoff (without it the long cases have margins of the order of eps);
* roundoff_eps  the fp32 error bound of a score path, elem_eps that of one emission;
* CASES / case_inputs   the inputs of tests/test_gpu_ctc_align.py, pinned decidable by test_ctc_align_ref_cpu.py."""
import itertools
import math

import numpy as np

from tests.ctc_beam_ref import log_softmax, make_logits

NEG = -np.inf


def ext_labels(target, blank=0):
    ext = [blank]
    for c in target:
        ext += [int(c), blank]
    return np.asarray(ext, np.int64)


def repeats(target):
    return sum(1 for a, c in zip(target, target[1:]) if a == c)


def feasible(T, target):
    return T >= len(target) + repeats(target)


def _skip_mask(ext):
    S = len(ext)
    ok = np.zeros(S, bool)
    for s in range(3, S, 2):
        ok[s] = ext[s] != ext[s - 2]
    return ok


def _down(v, k):
    """out[s] = v[s - k] (-inf below state 0)."""
    return np.concatenate([np.full(k, NEG), v])[:len(v)]


def _up(v, k):
    """out[s] = v[s + k] (-inf above the last state)."""
    return np.concatenate([v[k:], np.full(k, NEG)])[:len(v)]


def viterbi(lp, target, blank=0):
    """lp (T, V) fp64 -> (state path (T,) int array, score), or (None, -inf) when infeasible."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    if not feasible(T, target):
        return None, NEG
    if T == 0:
        return np.zeros(0, np.int64), 0.0
    ext = ext_labels(target, blank)
    S = len(ext)
    skip = _skip_mask(ext)
    em = lp[:, ext]                                          # (T, S)
    v = np.full(S, NEG)
    v[:2] = em[0, :2]
    mv = np.zeros((T, S), np.int8)
    for t in range(1, T):
        n1 = _down(v, 1)
        n2 = np.where(skip, _down(v, 2), NEG)
        best = v.copy()
        take1 = n1 > best                                    # strictly better only: stay wins a tie
        best = np.where(take1, n1, best)
        take2 = n2 > best
        best = np.where(take2, n2, best)
        mv[t] = np.where(take2, 2, np.where(take1, 1, 0))
        v = best + em[t]
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:                       # the final blank wins a tie
        s = S - 2
    score = float(v[s])
    if not score > NEG:
        return None, NEG
    path = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(mv[t, s])
    return path, score


def _collapse(lab, blank):
    out, prev = [], None
    for c in lab:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def _states_of(lab, blank):
    """The state path of a labelling that collapses to its target."""
    s, prev, out = 0, None, []
    for c in lab:
        if c == blank:
            s += s & 1
        elif not (s & 1 and c == prev):
            s += 1 if s % 2 == 0 else 2
        out.append(s)
        prev = c
    return out


def brute_force(lp, target, blank=0, through=False):
    """Enumerates all V^T labellings -> (state path of a best one, its score), (None, -inf) if none collapses to the
    target; through=True: also the (T, S) table of the best score of any alignment through each cell."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    S = 2 * len(target) + 1
    best, best_path = NEG, None
    table = np.full((T, S), NEG)
    target = [int(c) for c in target]
    for lab in itertools.product(range(V), repeat=T):
        if _collapse(lab, blank) != target:
            continue
        sc = float(sum(lp[t, c] for t, c in enumerate(lab)))
        st = _states_of(lab, blank)
        if sc > best:
            best, best_path = sc, np.asarray(st, np.int64)
        for t, s in enumerate(st):
            table[t, s] = max(table[t, s], sc)
    if T == 0 and not target:
        best, best_path = 0.0, np.zeros(0, np.int64)
    return (best_path, best, table) if through else (best_path, best)


def through_table(lp, target, blank=0):
    """(T, S): the score of the best alignment through each cell (-inf: none)."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    ext = ext_labels(target, blank)
    S = len(ext)
    skip = _skip_mask(ext)
    em = lp[:, ext]
    fwd = np.full((T, S), NEG)
    bwd = np.full((T, S), NEG)
    if T == 0:
        return fwd
    fwd[0, :2] = em[0, :2]
    for t in range(1, T):
        v = fwd[t - 1]
        n1 = _down(v, 1)
        n2 = np.where(skip, _down(v, 2), NEG)
        fwd[t] = np.maximum(np.maximum(v, n1), n2) + em[t]
    bwd[T - 1, max(S - 2, 0):] = 0.0
    for t in range(T - 2, -1, -1):
        w = bwd[t + 1] + em[t + 1]                           # entering state s' at frame t + 1
        up1 = _up(w, 1)                                      # s -> s + 1
        up2 = _up(np.where(skip, w, NEG), 2)                 # s -> s + 2 where s + 2 may be skipped into
        bwd[t] = np.maximum(np.maximum(w, up1), up2)
    return fwd + bwd


def margin(lp, target, blank=0):
    """The smallest gap, over the frames, between the best and the runner-up state of through_table (inf: nowhere a
    second state, or nothing to align)."""
    th = through_table(lp, target, blank)
    gap = np.inf
    for row in th:
        top = np.sort(row)[::-1]
        if not top[0] > NEG:
            return np.inf
        if len(top) > 1 and top[1] > NEG:
            gap = min(gap, float(top[0] - top[1]))
    return gap


def random_alignment(T, target, rng, blank=0):
    """A random valid state path of T frames, or None when the target is infeasible."""
    L = len(target)
    if not feasible(T, target) or T == 0:
        return None
    must = [1]
    for u in range(1, L):
        if target[u] == target[u - 1]:
            must.append(2 * u)
        must.append(2 * u + 1)
    if L == 0:
        must = [0]
    optional = [s for s in range(0, 2 * L + 1, 2) if s not in must]
    room = T - len(must)
    rng.shuffle(optional)
    extra = [s for s in optional[:room] if rng.random() < 0.5]
    visit = sorted(must + extra)
    dur = np.ones(len(visit), np.int64)
    for k in rng.integers(0, len(visit), T - len(visit)):
        dur[k] += 1
    return np.repeat(np.asarray(visit, np.int64), dur)


def plant(x, target, rng, boost, blank=0):
    """x (T, V) logits -> a copy with `boost` added to the logit of a random valid alignment's label at each frame
    (unchanged where the target is infeasible)."""
    x = np.array(x, copy=True)
    path = random_alignment(x.shape[0], target, rng, blank)
    if path is not None:
        ext = ext_labels(target, blank)
        x[np.arange(x.shape[0]), ext[path]] += np.float32(boost)
    return x


def roundoff_eps(T, max_abs_score):
    """k T 2^-24 max(1, |score|) with k = 4 fp32 roundings per frame on a score path of the kernels as built
    (align_prep: lpe = (x[label] - m) - log(sum exp(x - m)); align_viterbi: v = max(...) + lpe):
      1  x[label] - m;
      2  log(sum): the logarithm's rounding, and the sum's relative error, which is an absolute error of its
         logarithm (all terms positive and the largest exactly 1, so the sum is in [1, V] with no cancellation);
      3  the subtraction of the two;
      4  the recursion's add (the max itself is exact).
    The terms of lpe are both <= 0, so |x - m|, log(sum) and |lpe| are each at most |lpe|, and with every emission
    <= 0 each |lpe| and each partial sum is at most |score|: every rounding is at most 2^-24 max(1, |score|), the 1
    covering the sum's error where the score is small.  (Through lse = m + log(sum) the roundings would scale with
    |lse| instead, which no multiple of |score| bounds for raw logits.)  The beam decoder's tests count 4 as well."""
    return 4.0 * T * 2.0 ** -24 * max(1.0, max_abs_score)


def elem_eps(V, lp_abs):
    """Bound of |scores[b, t] - lp[t, label]| for one emission (x[label] - m) - log(sum exp(x - m)) of align_prep, in
    units of 2^-24:
      x - m before each exponential   a relative error |x - m| 2^-24 of that term; weighted by the softmax the terms'
                                      |x - m| average to at most ln V                                    ln V
      expf, 1 ulp                     2 (relative, of the sum)
      the sum                         ceil(V / 64) sequential adds per lane + 6 shuffle steps, all terms positive
      logf, 1 ulp of a value in [0, ln V]                                                                2 ln V
      x[label] - m and the final subtraction, each at most |lp|                                          2 |lp|"""
    return 2.0 ** -24 * (3.0 * math.log(V) + 2 + math.ceil(V / 64) + 6 + 2.0 * lp_abs)


# ----------------------------------------------------------------------------- the GPU test's inputs
# name: (seed, B, T, V, scale, [(target lengths, input lengths or None), ...]); each entry of the list is one call
# with logits of its own.  every_third: every third label repeats its predecessor.
CASES = {
    "ragged_empty_infeasible": (21, 4, 33, 5, 2.0, [((6, 1, 0, 16), (33, 1, 0, 17))]),
    "repeats_tight": (22, 3, 24, 4, 2.0, [((12, 8, 11), (17, 11, 24))]),
    "one_wave_edge": (23, 2, 160, 40, 3.0, [((31, 32), (160, 131)), ((31, 30), (160, 131))]),
    "two_wave_edge": (37, 2, 300, 40, 3.0, [((63, 64), (300, 283)), ((100, 129), (300, 283))]),
    "limit": (25, 1, 530, 8, 2.0, [((511,), None)]),
    "v1024": (26, 2, 48, 1024, 3.0, [((20, 5), (48, 31))]),
    "v2_t1": (27, 2, 1, 2, 2.0, [((1, 0), None)]),
}


def make_target(rng, L, V, name, blank=0):
    """L labels in [1, V): `repeats_tight` repeats every third label; the 16-label row of `ragged_empty_infeasible`
    gets two repeats (16 + 2 > its 17 frames); `limit` has five repeats in 511 labels (516 <= 530 frames); the others
    are free draws without adjacent repeats."""
    assert blank == 0
    out = []
    for u in range(L):
        c = int(rng.integers(1, V))
        while V > 2 and out and c == out[-1]:
            c = int(rng.integers(1, V))
        out.append(c)
    rep = []
    if name == "repeats_tight":
        rep = range(2, L, 3)
    elif name == "ragged_empty_infeasible" and L == 16:
        rep = (5, 11)
    elif name == "limit":
        rep = (40, 140, 260, 400, 510)
    for u in rep:
        out[u] = out[u - 1]
        if u + 1 < L and V > 2:
            while out[u + 1] == out[u] or (u + 2 < L and out[u + 1] == out[u + 2]):
                out[u + 1] = int(rng.integers(1, V))
    return out


def case_inputs(name):
    """-> [(x (B, T, V) fp32 planted logits, targets: B lists, input lengths: B ints)] per call of the case."""
    seed, B, T, V, scale, calls = CASES[name]
    out = []
    for k, (tls, ils) in enumerate(calls):
        rng = np.random.default_rng(1000 * seed + k)
        x = make_logits(100 * seed + k, B, T, V, scale)
        ils = [T] * B if ils is None else list(ils)
        targets = [make_target(rng, L, V, name) for L in tls]
        for b in range(B):
            x[b, :ils[b]] = plant(x[b, :ils[b]], targets[b], rng, 3.0 * scale)
        out.append((x, targets, ils))
    return out


def spans_of(path, scores, L):
    """Host recomputation of the spans: path is the per-frame state path (T_b,), scores the per-frame scores ->
    (starts, ends, token sums accumulated in frame order in fp32) for u < L."""
    starts, ends, sums = [-1] * L, [-1] * L, [np.float32(0.0)] * L
    for t, s in enumerate(path):
        if s & 1:
            u = int(s) >> 1
            if starts[u] < 0:
                starts[u] = t
            ends[u] = t + 1
            sums[u] = np.float32(sums[u] + np.float32(scores[t]))
    return starts, ends, [float(v) for v in sums]


def states_from_labels(labels, target, blank=0):
    """The state path of a per-frame label sequence claimed to align `target`, checking on the way that it is a valid
    alignment: monotone with steps 0 / 1 / 2, a step of 2 only over a blank between different labels, start in state
    0 or 1, end in S - 1 or S - 2, collapsing to the target.  Raises AssertionError otherwise."""
    labels = [int(c) for c in labels]
    target = [int(c) for c in target]
    assert _collapse(labels, blank) == target, "the labels do not collapse to the target"
    st = _states_of(labels, blank)
    ext = ext_labels(target, blank)
    S = len(ext)
    if st:
        assert st[0] in (0, 1) and st[-1] in (S - 1, max(S - 2, 0))
    for t, s in enumerate(st):
        assert 0 <= s < S and ext[s] == labels[t]
        if t:
            d = s - st[t - 1]
            assert d in (0, 1, 2)
            if d == 2:
                assert s & 1 and ext[s] != ext[s - 2]
    return np.asarray(st, np.int64)
