"""Integer restatement of the edit-distance contract of include/cfm.h (cfm_edit_distance) in numpy, pinned on the CPU
by tests/test_edit_distance_ref_cpu.py and used as the reference of tests/test_gpu_edit_distance.py.

  table(r, h)        D, (R + 1, H + 1): D[i][0] = i, D[0][j] = j,
                     D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
  directions(r, h)   per cell i, j >= 1 the FIRST of diagonal (0), up (1), left (2) that attains the minimum
  align(r, h)        the one path from (R, H) under that rule (i == 0 walks left, j == 0 walks up): distance,
                     counts (hits, subs, dels, ins) and the pairs in forward order, -1 on the gap side
  brute_force(r, h)  the minimum cost over all monotone edit scripts by exhaustive recursion (no table)
  CASES / case(name) the batches of the GPU test: the smallest shapes at which each mechanism of the kernel (one
                     strip of 64 reference rows without LDS, several strips with the carried row, the 16-step
                     direction words, the borders) can go wrong.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

Alignment = namedtuple("Alignment", "distance counts pair_ref pair_hyp")


def table(r, h):
    r, h = np.asarray(r, dtype=np.int64), np.asarray(h, dtype=np.int64)
    R, H = len(r), len(h)
    D = np.zeros((R + 1, H + 1), dtype=np.int64)
    D[0] = np.arange(H + 1)
    D[:, 0] = np.arange(R + 1)
    cols = np.arange(1, H + 1)
    for i in range(1, R + 1):
        # x[j] = min(diagonal, up); D[i][j] = min(x[j], D[i][j-1] + 1) = min over k <= j of x[k] + (j - k), with
        # x[0] = D[i][0]: a running minimum of x[k] - k
        x = np.minimum(D[i - 1, :-1] + (r[i - 1] != h), D[i - 1, 1:] + 1)
        D[i, 1:] = np.minimum.accumulate(np.concatenate(([i], x - cols)))[1:] + cols
    return D


def directions(r, h, D=None):
    """(R + 1, H + 1) int8, meaningful for i, j >= 1; also the number of cells where two predecessors tie."""
    r, h = np.asarray(r, dtype=np.int64), np.asarray(h, dtype=np.int64)
    D = table(r, h) if D is None else D
    diag = D[:-1, :-1] + (r[:, None] != h[None, :])
    up = D[:-1, 1:] + 1
    left = D[1:, :-1] + 1
    best = D[1:, 1:]
    assert np.array_equal(best, np.minimum(np.minimum(diag, up), left))
    d = np.where(diag == best, 0, np.where(up == best, 1, 2)).astype(np.int8)
    ties = int((((diag == best).astype(int) + (up == best) + (left == best)) >= 2).sum())
    out = np.zeros(D.shape, dtype=np.int8)
    out[1:, 1:] = d
    return out, ties


def align(r, h):
    r, h = [int(x) for x in r], [int(x) for x in h]
    D = table(r, h)
    dirs, _ = directions(r, h, D)
    i, j = len(r), len(h)
    pr, ph = [], []
    hits = subs = dels = ins = 0
    while i > 0 or j > 0:
        mv = 2 if i == 0 else 1 if j == 0 else int(dirs[i, j])
        if mv == 0:
            pr.append(r[i - 1]); ph.append(h[j - 1])
            hits += r[i - 1] == h[j - 1]
            subs += r[i - 1] != h[j - 1]
            i, j = i - 1, j - 1
        elif mv == 1:
            pr.append(r[i - 1]); ph.append(-1)
            dels += 1
            i -= 1
        else:
            pr.append(-1); ph.append(h[j - 1])
            ins += 1
            j -= 1
    return Alignment(int(D[-1, -1]), (hits, subs, dels, ins), pr[::-1], ph[::-1])


def brute_force(r, h):
    r, h = list(r), list(h)
    if not r:
        return len(h)
    if not h:
        return len(r)
    return min(brute_force(r[1:], h[1:]) + (r[0] != h[0]), brute_force(r[1:], h) + 1, brute_force(r, h[1:]) + 1)


# ----------------------------------------------------------------------------- the GPU test's cases
SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 70), (64, 64), (65, 3), (127, 129), (128, 128), (129, 127), (200, 1),
          (1, 200), (1023, 1024), (1024, 1023)]


def _related(rng, R, H, V):
    """A reference of R ids below V and a hypothesis of H ids made from it by random edits (so the alignment has
    hits, substitutions, deletions and insertions even over a large vocabulary)."""
    r = rng.integers(0, V, R)
    out = []
    for t in r:
        u = rng.random()
        if u < 0.1:
            continue
        out.append(int(rng.integers(0, V)) if u < 0.25 else int(t))
        if rng.random() < 0.1:
            out.append(int(rng.integers(0, V)))
    out = out[:H] + [int(x) for x in rng.integers(0, V, max(0, H - len(out)))]
    return r.astype(np.int64), np.asarray(out, dtype=np.int64)


def _shapes(shapes, V, seed):
    rng = np.random.default_rng(seed)
    return [_related(rng, R, H, V) for R, H in shapes]


def _special():
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 1024, 65), rng.integers(0, 9, 5)
    rep = np.full(128, 7)
    return [(a, a.copy()), (b, b.copy()),                                                    # identical
            (rng.integers(0, 500, 63), rng.integers(500, 1000, 70)),                         # disjoint alphabets
            (rng.integers(0, 500, 129), rng.integers(500, 1000, 127)),
            (rep, rng.integers(7, 9, 128)), (rng.integers(7, 9, 70), np.full(60, 7))]        # one repeated token


# name -> (what the case is for, builder).  B is 1 to 7; every batch but the single pair mixes references of at most
# 64 ids (one strip) with longer ones, so one launch holds both kernel paths.
CASES = {
    "small_v2": ("borders, one strip / two strips, ties", lambda: _shapes(SHAPES[:7], 2, 1)),
    "small_v1024": ("borders, one strip / two strips", lambda: _shapes(SHAPES[:7], 1024, 2)),
    "mid_v2": ("strip boundaries at 128, ties", lambda: _shapes(SHAPES[7:12], 2, 3)),
    "mid_v1024": ("strip boundaries at 128", lambda: _shapes(SHAPES[7:12], 1024, 4)),
    "long_v2": ("the largest sizes, ties", lambda: _shapes(SHAPES[12:] + [(1, 1)], 2, 5)),
    "long_v1024": ("the largest sizes", lambda: _shapes(SHAPES[12:] + [(64, 64)], 1024, 6)),
    "single": ("a batch of one pair", lambda: _shapes([(64, 64)], 1024, 8)),
    "special": ("identical, disjoint, repeated token", _special),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pairs [(r, h), ...], alignments [Alignment, ...]); computed once per process and shared: do not modify."""
    pairs = [(np.asarray(r, dtype=np.int64), np.asarray(h, dtype=np.int64)) for r, h in CASES[name][1]()]
    return pairs, [align(r, h) for r, h in pairs]
