"""cfm_adafactor_plan: what every parameter of a group contributes to each launch of the Adafactor step, and where
its share begins, pinned without a GPU.  cfm_adafactor_fill_table writes the table through the same routine
(csrc/ada_plan.h) and cfm_adafactor_step sizes its grids from the totals, so these rows are the launches.  The
expectations are typed in from the rule as ada_plan.h and include/cfm.h state it and worked out by hand in the comments."""
import ctypes

import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib as L
from nn_conformer_for_speech_recognition_amd.optim import Adafactor

TOTAL = [n for n, _ in L.AdafactorTotals._fields_]      # row_tasks cols blocks rowmean_tasks colpart_tasks + 2 sizes
# a parameter's offsets in the table (optim.hip, AdaP) are the totals in front of it, under these names
SLOT = dict(row_toff="row_tasks", col_off="cols", blk_off="blocks", rm_off="rowmean_floats", rm_toff="rowmean_tasks",
            cp_toff="colpart_tasks", part_off="part_floats")


def _params(shapes, pointers=False):
    """The geometry optim.Adafactor gives these shapes; the plan never reads the pointers."""
    ps = (L.AdafactorParam * len(shapes))()
    for q, shape in zip(ps, shapes):
        factored, q.nb, q.R, q.C = Adafactor._geom(torch.empty(shape, device="meta"))
        q.factored, q.numel = factored, torch.Size(shape).numel()
        if pointers:        # (never dereferenced on the host)
            q.p, q.g, q.row, q.col = 0x1000, 0x2000, 0x3000, 0x4000 if factored else None
    return ps


def _plan(shapes):
    ps, before, tot = _params(shapes), (L.AdafactorTotals * len(shapes))(), L.AdafactorTotals()
    L.call("cfm_adafactor_plan", ps, len(shapes), before, ctypes.byref(tot))
    return ps, [{k: getattr(b, v) for k, v in SLOT.items()} for b in before], {k: getattr(tot, k) for k in TOTAL}


# The shape list of tests/test_gpu_adafactor_full.py (SHAPES + (64,) + (24, 40)), in its order.  A shape (..., R, C)
# is nb = prod(...) matrices; CHUNK 4096, RB 32, ROWS_PER_TASK 256, wide: 64 <= C <= 2560.  Per entry:
#   (row tasks, cols, blocks, rowmean tasks, colpart tasks, rowmean floats, part floats)
TABLE = [
    ((37,), (0, 0, 1, 0, 0, 0, 0)),               # unfactored: only blocks, ceil(37 / 4096)
    ((5,), (0, 0, 1, 0, 0, 0, 0)),
    ((4096,), (0, 0, 1, 0, 0, 0, 0)),
    ((4097,), (0, 0, 2, 0, 0, 0, 0)),
    # narrow (C 48 < 64): 64 rows -> ceil(64 / 256) = 1 row task; R >= 64: a row-mean wave per matrix; 3072 el.
    ((64, 48), (1, 48, 1, 1, 0, 1, 0)),
    # wide: ceil(300 / 32) = 10 row blocks, 10 * 2304 partials; 691200 / 4096 = 168.75 -> 169
    ((300, 2304), (0, 2304, 169, 1, 10, 1, 23040)),
    # C 3000 > 2560, past the wide limit: 33 rows -> 1 row task; R < 64: ceil(1 / 64) = 1; 99000 / 4096 = 24.2 -> 25
    ((33, 3000), (1, 3000, 25, 1, 0, 1, 0)),
    # nb 128, R 3, C 3: 384 rows -> 2 row tasks; 128 * 3 columns; 128 row means, 64 matrices per wave -> 2
    ((16, 8, 3, 3), (2, 384, 1, 2, 0, 128, 0)),
    ((8, 16, 1), (1, 8, 1, 1, 0, 8, 0)),          # nb 8, R 16, C 1: 128 rows -> 1; 8 columns; 8 means in 1 wave
    # nb 2, R 70, C 100: wide, 2 * ceil(70 / 32) = 6 tasks of 100 partials; R >= 64: 2 row-mean waves; 14000 el. -> 4
    ((2, 70, 100), (0, 200, 4, 2, 6, 2, 600)),
    ((64,), (0, 0, 1, 0, 0, 0, 0)),
    ((24, 40), (1, 40, 1, 1, 0, 1, 0)),           # narrow, R < 64
]
SHAPES = [s for s, _ in TABLE]
# sums of the columns above: 1+1+2+1+1 | 48+2304+3000+384+8+200+40 | 5+169+25+1+1+4+1+1+1 | 1+1+1+2+1+2+1 | 10+6 |
# 1+1+1+128+8+2+1 | 23040+600
TOTALS = dict(row_tasks=6, cols=5984, blocks=208, rowmean_tasks=9, colpart_tasks=16, rowmean_floats=142,
              part_floats=23640)
# the running sums in front of each entry: (row_toff, col_off, blk_off, rm_off, rm_toff, cp_toff, part_off)
SLOTS = [
    (0, 0, 0, 0, 0, 0, 0),
    (0, 0, 1, 0, 0, 0, 0),
    (0, 0, 2, 0, 0, 0, 0),
    (0, 0, 3, 0, 0, 0, 0),
    (0, 0, 5, 0, 0, 0, 0),                        # (64, 48)
    (1, 48, 6, 1, 1, 0, 0),                       # (300, 2304)
    (1, 2352, 175, 2, 2, 10, 23040),              # (33, 3000)
    (2, 5352, 200, 3, 3, 10, 23040),              # (16, 8, 3, 3)
    (4, 5736, 201, 131, 5, 10, 23040),            # (8, 16, 1)
    (5, 5744, 202, 139, 6, 10, 23040),            # (2, 70, 100)
    (5, 5944, 206, 141, 8, 16, 23640),            # (64,)
    (5, 5944, 207, 141, 8, 16, 23640),            # (24, 40)
]


def test_totals_and_slots_of_the_gpu_tests_shapes():
    _, slots, tot = _plan(SHAPES)
    assert tot == TOTALS
    assert [tuple(s[k] for k in SLOT) for s in slots] == SLOTS
    # the typed-in rows are consistent: each planned alone gives its row, and the slots are their running sums
    run = dict.fromkeys(TOTAL, 0)
    for (shape, row), slot in zip(TABLE, slots):
        assert _plan([shape])[2] == dict(zip(TOTAL, row)), shape
        assert slot == dict(row_toff=run["row_tasks"], col_off=run["cols"], blk_off=run["blocks"],
                            rm_off=run["rowmean_floats"], rm_toff=run["rowmean_tasks"], cp_toff=run["colpart_tasks"],
                            part_off=run["part_floats"]), shape
        for k, v in zip(TOTAL, row):
            run[k] += v


def test_fill_table_plans_the_same():
    """cfm_adafactor_fill_table returns the plan's totals (and needs the pointers the plan does not)."""
    ps, tot = _params(SHAPES, pointers=True), L.AdafactorTotals()
    host = (ctypes.c_char * L.size_call("cfm_adafactor_table_bytes", len(SHAPES)))()
    L.call("cfm_adafactor_fill_table", ctypes.cast(host, ctypes.c_void_p), ps, len(SHAPES), ctypes.byref(tot))
    assert {k: getattr(tot, k) for k in TOTAL} == TOTALS
    with pytest.raises(L.CfmError, match="null pointer"):
        L.call("cfm_adafactor_fill_table", ctypes.cast(host, ctypes.c_void_p), _params(SHAPES), len(SHAPES),
               ctypes.byref(tot))


# The kernels' parameter search (optim.hip, find_param): the owner of item i of a phase is the last entry whose
# offset of that phase is <= i.  (phase: its offset, its total, must its owner be factored)
PHASES = [("row_toff", "row_tasks", True), ("col_off", "cols", True), ("blk_off", "blocks", False),
          ("rm_toff", "rowmean_tasks", True), ("cp_toff", "colpart_tasks", True)]
MIXED = [(70, 100), (5,), (64, 48), (300,), (2, 70, 100), (4097,), (37,), (24, 40), (33, 3000), (128, 64), (64,)]
# by hand, as TABLE: (row tasks, cols, blocks, rowmean tasks, colpart tasks, rowmean floats, part floats)
MIXED_ROWS = [
    (0, 100, 2, 1, 3, 1, 300),          # (70, 100) wide: ceil(70 / 32) = 3 tasks of 100 partials; 7000 el. -> 2
    (0, 0, 1, 0, 0, 0, 0),              # (5,)
    (1, 48, 1, 1, 0, 1, 0),             # (64, 48) narrow
    (0, 0, 1, 0, 0, 0, 0),              # (300,)
    (0, 200, 4, 2, 6, 2, 600),          # (2, 70, 100)
    (0, 0, 2, 0, 0, 0, 0),              # (4097,)
    (0, 0, 1, 0, 0, 0, 0),              # (37,)
    (1, 40, 1, 1, 0, 1, 0),             # (24, 40)
    (1, 3000, 25, 1, 0, 1, 0),          # (33, 3000)
    (0, 64, 2, 1, 4, 1, 256),           # (128, 64) wide at the lower limit: 4 row blocks of 64; 8192 el. -> 2
    (0, 0, 1, 0, 0, 0, 0),              # (64,)
]
UNFACTORED = [(37,), (4096,), (4097,), (5,)]


def _owner(offs, i):
    lo, hi = 0, len(offs) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if offs[mid] <= i:
            lo = mid
        else:
            hi = mid - 1
    return lo


@pytest.mark.parametrize("shapes", [SHAPES, MIXED, UNFACTORED], ids=["gpu-tests", "interleaved", "unfactored-only"])
def test_every_item_is_owned_by_a_parameter_that_has_it(shapes):
    """What the kernels rely on: an entry with no items of a phase is never found by that phase's search, and the
    entry that is found covers the item."""
    ps, slots, tot = _plan(shapes)
    alone = [_plan([s])[2] for s in shapes]         # what each entry contributes by itself
    if shapes is MIXED:
        assert [tuple(a[k] for k in TOTAL) for a in alone] == MIXED_ROWS
    for off, total, must_be_factored in PHASES:
        offs = [s[off] for s in slots]
        for i in range(tot[total]):
            o = _owner(offs, i)
            assert alone[o][total] >= 1, (off, i, shapes[o])
            assert offs[o] <= i < offs[o] + alone[o][total], (off, i, shapes[o])
            assert ps[o].factored or not must_be_factored, (off, i, shapes[o])
    if shapes is UNFACTORED:
        assert tot == dict(dict.fromkeys(TOTAL, 0), blocks=5)      # 1 + 1 + 2 + 1: nothing but blocks
    if shapes is MIXED:     # zero-task entries do sit between owners: wide, unfactored, narrow interleaved
        assert [a["colpart_tasks"] > 0 for a in alone] == [True, False, False, False, True, False, False, False,
                                                           False, True, False]
        assert [a["row_tasks"] > 0 for a in alone] == [False, False, True, False, False, False, False, True, True,
                                                       False, False]


def test_rejects_2_to_the_31_elements():
    ps, tot = _params([(8, 4), (4,)]), L.AdafactorTotals()
    ps[1].numel = ps[1].C = 2 ** 31 - 1
    L.call("cfm_adafactor_plan", ps, 2, None, ctypes.byref(tot))      # the largest tensor the 32-bit indices take
    assert tot.blocks == 1 + 2 ** 19
    ps[1].numel = 2 ** 31
    with pytest.raises(L.CfmError, match=r"tensor too large \(2\^31 elements\)"):
        L.call("cfm_adafactor_plan", ps, 2, None, ctypes.byref(tot))
    host = (ctypes.c_char * L.size_call("cfm_adafactor_table_bytes", 2))()
    with pytest.raises(L.CfmError, match=r"tensor too large \(2\^31 elements\)"):
        L.call("cfm_adafactor_fill_table", ctypes.cast(host, ctypes.c_void_p), ps, 2, ctypes.byref(tot))
