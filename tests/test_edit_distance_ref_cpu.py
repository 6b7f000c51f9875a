"""tests/edit_distance_ref.py (the reference of the device edit distance, include/cfm.h cfm_edit_distance) pinned on
the CPU: against an exhaustive search that uses no table, against myvocab.wer on strings, by its identities, by
replaying its pairs, on hand-written tie cases, and on the GPU test's own cases (each must exercise what it says)."""
import itertools

import numpy as np
import pytest

from nn_conformer_for_speech_recognition_amd.lib.standard.myvocab import Vocab, wer
from tests import edit_distance_ref as er


def _replay(a):
    r = [x for x in a.pair_ref if x >= 0]
    h = [x for x in a.pair_hyp if x >= 0]
    return r, h


def _check_alignment(r, h, a):
    r, h = [int(x) for x in r], [int(x) for x in h]
    hits, subs, dels, ins = a.counts
    assert hits + subs + dels == len(r)
    assert hits + subs + ins == len(h)
    assert subs + dels + ins == a.distance
    assert _replay(a) == (r, h)
    assert len(a.pair_ref) == len(a.pair_hyp) <= len(r) + len(h)
    assert all(x >= 0 or y >= 0 for x, y in zip(a.pair_ref, a.pair_hyp))
    assert sum(x != y for x, y in zip(a.pair_ref, a.pair_hyp)) == a.distance
    assert sum(x == y for x, y in zip(a.pair_ref, a.pair_hyp)) == hits


def test_table_matches_exhaustive_search():
    seqs = [s for n in range(5) for s in itertools.product(range(3), repeat=n)]
    assert len(seqs) == 1 + 3 + 9 + 27 + 81
    for r in seqs:
        for h in seqs:
            assert er.table(r, h)[-1, -1] == er.brute_force(r, h), (r, h)


def test_table_recurrence_cell_by_cell():
    rng = np.random.default_rng(0)
    for _ in range(20):
        r, h = rng.integers(0, 3, rng.integers(0, 12)), rng.integers(0, 3, rng.integers(0, 12))
        D = er.table(r, h)
        assert list(D[0]) == list(range(len(h) + 1)) and list(D[:, 0]) == list(range(len(r) + 1))
        for i in range(1, len(r) + 1):
            for j in range(1, len(h) + 1):
                assert D[i, j] == min(D[i - 1, j - 1] + (r[i - 1] != h[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)


def test_distance_matches_wer_on_strings():
    voc = Vocab(["<blank>", "<pad>"] + [f"w{i}" for i in range(6)])
    rng = np.random.default_rng(1)
    for _ in range(200):
        r = rng.integers(2, 8, rng.integers(1, 20)).tolist()
        h = rng.integers(2, 8, rng.integers(0, 20)).tolist()
        rs, hs = voc.decode([r])[0], voc.decode([h])[0]
        a = er.align(r, h)
        assert a.distance == round(wer(rs, hs) * len(r))
        assert a.distance == er.table(r, h)[-1, -1]
        _check_alignment(r, h, a)


A, B, C = 10, 11, 12
TIES = [
    # r, h, pairs (ref side, hyp side) in forward order
    ([A, B], [B, A], [(A, B), (B, A)]),                      # two substitutions beat deletion + hit + insertion
    ([A, A, A], [A], [(A, -1), (A, -1), (A, A)]),            # diagonal wins the ties: the LAST token is the hit
    ([A], [A, A, A], [(-1, A), (-1, A), (A, A)]),
    ([], [A, B], [(-1, A), (-1, B)]),
    ([A, B], [], [(A, -1), (B, -1)]),
    ([], [], []),
    ([A, B], [A], [(A, A), (B, -1)]),                        # (2,1): diagonal costs 1 + 1, up costs 0 + 1: up
    ([A], [B, A], [(-1, B), (A, A)]),
    ([A, B, C], [A, C], [(A, A), (B, -1), (C, C)]),
]


@pytest.mark.parametrize("r,h,pairs", TIES)
def test_hand_written_tie_cases(r, h, pairs):
    a = er.align(r, h)
    assert list(zip(a.pair_ref, a.pair_hyp)) == pairs
    _check_alignment(r, h, a)


def test_hand_written_cases_do_tie():
    for r, h in (([A, B], [B, A]), ([A, A, A], [A]), ([A], [A, A, A])):
        assert er.directions(r, h)[1] >= 1


@pytest.mark.parametrize("name", sorted(er.CASES))
def test_gpu_cases_exercise_what_they_say(name):
    pairs, aligns = er.case(name)
    assert 1 <= len(pairs) <= 7
    shapes = [(len(r), len(h)) for r, h in pairs]
    for (r, h), a in zip(pairs, aligns):
        _check_alignment(r, h, a)
        assert max(len(r), len(h)) <= 1024
    if name != "single":      # both kernel paths in one launch: one strip (no LDS) and several strips
        assert any(R <= 64 for R, _ in shapes) and any(R > 64 for R, _ in shapes)
    if name.endswith("_v2"):
        for (r, h), (R, H) in zip(pairs, shapes):
            assert set(r.tolist()) | set(h.tolist()) <= {0, 1}
            if R >= 2 and H >= 2:
                assert er.directions(r, h)[1] >= 1, "a two-symbol case must have tied predecessors"
    if name.endswith("_v1024"):
        assert max(int(r.max(initial=0)) for r, _ in pairs) > 255      # ids need more than a byte
        if name != "single":
            assert any(min(a.counts) > 0 for a in aligns), "hits, substitutions, deletions and insertions in one path"
    if name == "special":
        assert [a.distance for a in aligns[:2]] == [0, 0] and all(len(r) > 0 for r, _ in pairs[:2])
        for (r, h), a in zip(pairs[2:4], aligns[2:4]):
            assert not set(r.tolist()) & set(h.tolist()) and a.distance == max(len(r), len(h))
        assert len(set(pairs[4][0].tolist())) == 1 and len(set(pairs[5][1].tolist())) == 1
    if name.startswith("long"):
        assert (1023, 1024) in shapes and (1024, 1023) in shapes


def test_gpu_cases_cover_every_shape():
    seen = {(len(r), len(h)) for name in er.CASES for r, h in er.case(name)[0]}
    assert set(er.SHAPES) <= seen
    for V in ("_v2", "_v1024"):
        seen_v = {(len(r), len(h)) for name in er.CASES if name.endswith(V) for r, h in er.case(name)[0]}
        assert set(er.SHAPES) <= seen_v
