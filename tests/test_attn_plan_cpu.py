"""cfm_attn_plan: which attention kernels a call runs and how the backward workspace is laid out, pinned without a
GPU.  cfm_attn_fwd, cfm_attn_bwd_ws_bytes and the backward call the same routine (csrc/attn_plan.h), so these rows are
the launches.  The expectations are typed in from the rule as include/cfm.h and DESIGN.md state it."""
import ctypes
from collections import namedtuple

import pytest

from nn_conformer_for_speech_recognition_amd import _lib as L

F32, BF16 = L.F32, L.BF16
SIMT, HEAD, TILED, REL = L.ATTN_PATH_SIMT, L.ATTN_PATH_HEAD, L.ATTN_PATH_TILED, L.ATTN_PATH_REL
NONE, XCD, R4V, R4 = L.ATTN_DPOS_NONE, L.ATTN_DPOS_XCD, L.ATTN_DPOS_R4_VEC, L.ATTN_DPOS_R4
M_TILED, M_RSIMT, M_ZERO = L.ATTN_MODE_TILED, L.ATTN_MODE_REL_SIMT, L.ATTN_MODE_REL_ZERO_FILL
M_R4, M_RDQ, M_DQ = L.ATTN_MODE_REL_DPOS_R4, L.ATTN_MODE_REL_DQ_RECOMPUTE, L.ATTN_MODE_DQ_RECOMPUTE


def _query(B, T, H, dk, dtype=BF16, rel=0, qkv=0, dout=0, pos=0, mode=0, cus=256, ws=-1):
    return L.AttnQuery(B, T, H, dk, dtype, rel, qkv, dout, pos, mode, cus, ws)


def _plan(q):
    c = L.AttnChoice()
    rc = L.load().cfm_attn_plan(ctypes.byref(q), ctypes.byref(c))
    return rc, c


# expected choice: path, vec, vec4, pvec, rel_vec, qs, waves, dq_stored, dpos
E = namedtuple("E", "path vec vec4 pvec rel_vec qs waves dq dpos")
E_SIMT = E(SIMT, 0, 0, 0, 0, 0, 0, 0, NONE)


def head(qs, waves, dq=1, vec=1, vec4=1):
    return E(HEAD, vec, vec4, 0, 0, qs, waves, dq, NONE)


def tiled(vec=1, vec4=1):
    return E(TILED, vec, vec4, 0, 0, 1, 0, 0, NONE)


def rel(vec=1, pvec=1, rel_vec=1, dq=1, dpos=XCD):
    return E(REL, vec, 0, pvec, rel_vec, 1, 0, dq, dpos)


# (query keywords, expected).  qs at 256 CUs: the largest q <= min(4, ceil(T/32)) with B*H*q <= 256; waves = ceil(ceil(T/32) / qs)
TABLE = [
    # ---- non-rel shapes of tests/test_gpu_attention.py, default mode and the mode each test sets
    (dict(B=3, T=373, H=2, dk=64), head(4, 3)),
    (dict(B=2, T=64, H=4, dk=64), head(2, 1)),                      # two 32-row blocks cap qs
    (dict(B=2, T=97, H=1, dk=64), head(4, 1)),
    (dict(B=3, T=373, H=2, dk=64, mode=M_TILED), tiled()),
    (dict(B=2, T=64, H=4, dk=64, mode=M_TILED), tiled()),
    (dict(B=2, T=97, H=1, dk=64, mode=M_TILED), tiled()),
    (dict(B=2, T=373, H=4, dk=64), head(4, 3)),
    (dict(B=3, T=97, H=2, dk=64), head(4, 1)),
    (dict(B=2, T=373, H=4, dk=36), head(4, 3, vec=0)),              # dk 36: 8-byte loads only
    (dict(B=1, T=384, H=2, dk=64), head(4, 3)),                     # HEAD_TMAX itself
    (dict(B=2, T=130, H=2, dk=64), head(4, 2)),                     # 5 blocks over 4 workgroups
    (dict(B=2, T=373, H=4, dk=64, mode=M_DQ), head(4, 3, dq=0)),
    (dict(B=3, T=97, H=2, dk=64, mode=M_DQ), head(4, 1, dq=0)),
    (dict(B=2, T=373, H=4, dk=36, mode=M_DQ), head(4, 3, dq=0, vec=0)),
    (dict(B=1, T=384, H=2, dk=64, mode=M_DQ), head(4, 3, dq=0)),
    (dict(B=2, T=130, H=2, dk=64, mode=M_DQ), head(4, 2, dq=0)),
    (dict(B=2, T=373, H=2, dk=64), head(4, 3)),
    (dict(B=2, T=373, H=2, dk=64, mode=M_TILED), tiled()),
    (dict(B=3, T=97, H=8, dk=64), head(4, 1)),
    (dict(B=2, T=64, H=2, dk=64), head(2, 1)),
    (dict(B=2, T=63, H=2, dk=64), head(2, 1)),
    (dict(B=2, T=37, H=2, dk=64), head(2, 1)),
    (dict(B=2, T=37, H=2, dk=64, mode=M_TILED), tiled()),
    (dict(B=2, T=97, H=2, dk=64), head(4, 1)),
    (dict(B=2, T=97, H=2, dk=64, mode=M_DQ), head(4, 1, dq=0)),
    (dict(B=2, T=130, H=2, dk=36), head(4, 2, vec=0)),
    (dict(B=2, T=130, H=2, dk=36, mode=M_DQ), head(4, 2, dq=0, vec=0)),
    (dict(B=2, T=130, H=2, dk=64, mode=M_TILED), tiled()),
    # ---- HEAD_TMAX: 384 whole-head, 385 tiled
    (dict(B=1, T=384, H=1, dk=64), head(4, 3)),
    (dict(B=1, T=385, H=1, dk=64), tiled()),
    # ---- alignment: 16-byte rows -> vec; 8-byte -> vec4 only; less -> neither; dout counts as qkv does
    (dict(B=2, T=97, H=2, dk=64, qkv=8), head(4, 1, vec=0)),
    (dict(B=2, T=97, H=2, dk=64, dout=8), head(4, 1, vec=0)),
    (dict(B=2, T=97, H=2, dk=64, qkv=4), head(4, 1, vec=0, vec4=0)),
    (dict(B=2, T=97, H=2, dk=36, qkv=8), head(4, 1, vec=0)),
    (dict(B=2, T=97, H=2, dk=30), head(4, 1, vec=0, vec4=0)),       # dk % 4 != 0
    # ---- the whole-head split at 256 CUs: qs = 1, 2, 3, 4 by B*H, the block cap, and one CU
    (dict(B=32, T=373, H=8, dk=64), head(1, 12)),                   # B*H = 256: one each
    (dict(B=43, T=373, H=3, dk=64), head(1, 12)),                   # B*H = 129: 258 > 256
    (dict(B=32, T=373, H=4, dk=64), head(2, 6)),                    # 128 * 2 = 256
    (dict(B=17, T=373, H=5, dk=64), head(3, 4)),                    # 85 * 3 = 255, 85 * 4 = 340
    (dict(B=16, T=373, H=4, dk=64), head(4, 3)),                    # 64 * 4 = 256
    (dict(B=1, T=32, H=1, dk=64), head(1, 1)),                      # one block: nothing to split
    (dict(B=1, T=65, H=1, dk=64), head(3, 1)),                      # three blocks cap qs
    (dict(B=2, T=97, H=2, dk=64, cus=1), head(1, 4)),
    (dict(B=2, T=373, H=2, dk=64, cus=8), head(2, 6)),
    (dict(B=2, T=97, H=2, dk=64, mode=M_ZERO), head(1, 4)),         # REL_ZERO_FILL: one workgroup per head
    # ---- fp32 and wide bf16 rel heads: SIMT
    (dict(B=1, T=37, H=2, dk=16, dtype=F32), E_SIMT),
    (dict(B=1, T=37, H=2, dk=16, dtype=F32, rel=1), E_SIMT),
    (dict(B=2, T=97, H=2, dk=64, dtype=F32), E_SIMT),
    (dict(B=1, T=37, H=2, dk=128, rel=1), E_SIMT),
    # ---- rel-pos shapes of tests/test_gpu_attention.py
    (dict(B=3, T=373, H=2, dk=64, rel=1), rel()),
    (dict(B=1, T=1498, H=2, dk=64, rel=1), rel()),
    (dict(B=2, T=1498, H=1, dk=64, rel=1), rel()),
    (dict(B=2, T=97, H=4, dk=36, rel=1), rel(vec=0, pvec=0, rel_vec=0, dpos=R4)),
    (dict(B=2, T=64, H=1, dk=64, rel=1), rel()),
    (dict(B=2, T=150, H=2, dk=64, rel=1), rel()),
    (dict(B=2, T=150, H=2, dk=64, rel=1, mode=M_RSIMT), E_SIMT),
    (dict(B=2, T=1498, H=3, dk=64, rel=1), rel()),
    (dict(B=9, T=130, H=2, dk=64, rel=1), rel()),
    (dict(B=2, T=1498, H=3, dk=64, rel=1, mode=M_R4), rel(dpos=R4V)),
    (dict(B=9, T=130, H=2, dk=64, rel=1, mode=M_R4), rel(dpos=R4V)),
    (dict(B=2, T=373, H=2, dk=64, rel=1), rel()),
    (dict(B=3, T=130, H=2, dk=64, rel=1), rel()),
    (dict(B=2, T=373, H=2, dk=64, rel=1, mode=M_RDQ), rel(dq=0)),
    (dict(B=3, T=130, H=2, dk=64, rel=1, mode=M_RDQ), rel(dq=0)),
    (dict(B=2, T=97, H=4, dk=64, rel=1), rel()),
    (dict(B=2, T=130, H=2, dk=64, rel=1), rel()),
    (dict(B=2, T=97, H=2, dk=36, rel=1), rel(vec=0, pvec=0, rel_vec=0, dpos=R4)),
    # ---- rel_vec off: a misaligned pos, qkv or dout; REL_ZERO_FILL; REL_DPOS_R4 without rel_vec stays non-vec
    (dict(B=2, T=130, H=2, dk=64, rel=1, pos=8), rel(pvec=0, rel_vec=0, dpos=R4)),
    (dict(B=2, T=130, H=2, dk=64, rel=1, qkv=8), rel(vec=0, rel_vec=0, dpos=R4)),
    (dict(B=2, T=130, H=2, dk=64, rel=1, dout=2), rel(vec=0, rel_vec=0, dpos=R4)),
    (dict(B=2, T=130, H=2, dk=64, rel=1, mode=M_ZERO), rel(rel_vec=0, dpos=R4)),
    (dict(B=2, T=130, H=2, dk=64, rel=1, mode=M_ZERO | M_R4), rel(rel_vec=0, dpos=R4)),
    (dict(B=2, T=97, H=2, dk=32, rel=1), rel(rel_vec=0, dpos=R4)),  # dk % 8 == 0 but not 64
    # ---- bits of the other family change nothing
    (dict(B=2, T=130, H=2, dk=64, rel=1, mode=M_TILED | M_DQ), rel()),
    (dict(B=2, T=130, H=2, dk=64, mode=M_RSIMT | M_R4 | M_RDQ), head(4, 2)),
]
IDS = ["-".join("%s%s" % kv for kv in kw.items()) for kw, _ in TABLE]


def _up(n):
    return (n + 255) // 256 * 256


def _sections(kw, e):
    """the layout restated from the comment in include/cfm.h: [(section, bytes)] in address order"""
    B, T, H, dk = kw["B"], kw["T"], kw["H"], kw["dk"]
    d = B * H * T * 4
    if e.path == SIMT:
        return [(L.ATTN_WS_DS, B * H * T * T * 4)]
    if e.path == REL:
        ldS = (T + 7) // 8 * 8
        return [(L.ATTN_WS_D, d), (L.ATTN_WS_PART, 4 * ((T + 127) // 128) * 2 * H * dk * 4 * B),
                (L.ATTN_WS_DS, B * H * T * ldS * 2), (L.ATTN_WS_DPOS, B * (2 * T - 1) * H * dk * 4)]
    if e.path == HEAD and e.dq:
        Tq = (T + 31) // 32 * 32
        return [(L.ATTN_WS_D, d), (L.ATTN_WS_DS, B * H * Tq * Tq * 2)]
    return [(L.ATTN_WS_D, d)]


def _total(sections):
    off = 0
    for _, n in sections:
        off = _up(off) + n           # every section but the last is rounded up to 256 bytes
    return off


@pytest.mark.parametrize("kw,want", TABLE, ids=IDS)
def test_choice_and_workspace(kw, want):
    lib = L.load()
    rc, c = _plan(_query(**kw))
    assert rc == 0, lib.cfm_get_last_error()
    got = E(c.path, c.vec, c.vec4, c.pvec, c.rel_vec, c.qs, c.waves, c.dq_stored, c.dpos)
    assert got == want
    # the timing bits reach only the non-rel MFMA kernels
    timing = L.ATTN_MODE_STAGING_ONLY | L.ATTN_MODE_SKIP_STORES
    rc, ct = _plan(_query(**dict(kw, mode=kw.get("mode", 0) | timing)))
    assert rc == 0 and c.dbg == 0 and ct.dbg == (timing if want.path in (HEAD, TILED) else 0)
    # layout: the sections the path has, in order, 256-aligned, not overlapping; total as restated
    secs = _sections(kw, want)
    assert [i for i in range(4) if c.ws_size[i]] == [i for i, _ in secs]
    end = 0
    for i, n in secs:
        assert c.ws_size[i] == n and c.ws_off[i] % 256 == 0 and c.ws_off[i] >= end and c.ws_off[i] < end + 256
        end = c.ws_off[i] + n
    assert c.ws_total == end == _total(secs)
    lib.cfm_attn_set_mode(kw.get("mode", 0))
    try:
        assert lib.cfm_attn_bwd_ws_bytes(kw["B"], kw["T"], kw["H"], kw["dk"], kw.get("rel", 0),
                                         kw.get("dtype", BF16)) == c.ws_total
    finally:
        lib.cfm_attn_set_mode(0)
    # offering exactly the need changes nothing; one byte less is an argument error
    rc, c2 = _plan(_query(**kw, ws=c.ws_total))
    assert rc == 0 and bytes(c2) == bytes(c)
    if want.path != HEAD or not want.dq:
        assert _plan(_query(**kw, ws=c.ws_total - 1))[0] == -1


def test_hand_computed_sizes():
    """numbers worked out on paper, not through _sections"""
    _, c = _plan(_query(2, 97, 2, 64))
    # D: 2*2*97*4 = 1552 -> dS^T at 1792; Tq = 128: 4 * 128 * 128 * 2 = 131072
    assert (c.ws_off[L.ATTN_WS_D], c.ws_size[L.ATTN_WS_D]) == (0, 1552)
    assert (c.ws_off[L.ATTN_WS_DS], c.ws_size[L.ATTN_WS_DS], c.ws_total) == (1792, 131072, 132864)
    _, c = _plan(_query(2, 97, 2, 64, mode=M_DQ))
    assert c.ws_total == 1552
    _, c = _plan(_query(1, 37, 2, 16, dtype=F32))
    assert c.ws_total == 2 * 37 * 37 * 4 == 10952 and c.ws_off[L.ATTN_WS_DS] == 0
    _, c = _plan(_query(2, 130, 2, 64, rel=1))
    # D 2080 -> 2304; partials 2 * 4*2 * 2*2*64 * 4 = 16384 -> 18688; dS 2*2*130*136*2 = 141440 -> 160256 (= 626 * 256);
    # dpos partials 2 * 259 * 128 * 4 = 265216
    assert list(c.ws_off) == [0, 2304, 18688, 160256] and list(c.ws_size) == [2080, 16384, 141440, 265216]
    assert c.ws_total == 425472
    # whole-head LDS at T 373 (12 blocks, 384 staged rows), 3 waves per workgroup: K+V images 2 * 384 * 144 B;
    # dK/dV: the images + 2 * 384 floats + 3 * 12 * 64 shorts; dQ-from-dS: 384 * 192 B of K + 3 * 4 KiB slices
    _, c = _plan(_query(3, 373, 2, 64))
    assert (c.lds_head, c.lds_dkdv, c.lds_dqs) == (110592, 118272, 86016)
    # one short block, one wave: the f32 output stage (32 * 65 * 4) is below every loop image
    _, c = _plan(_query(1, 20, 1, 64))
    assert (c.qs, c.waves, c.lds_head, c.lds_dkdv, c.lds_dqs) == (1, 1, 18432, 9600, 16384)
    _, c = _plan(_query(1, 385, 1, 64))
    assert (c.lds_head, c.lds_dkdv, c.lds_dqs) == (0, 0, 0)


def test_offered_bytes_decide_the_dq_source():
    B, T, H, dk = 2, 97, 2, 64
    d, full = B * H * T * 4, 132864
    for ws, dq, total in [(full, 1, full), (full + 4096, 1, full), (full - 1, 0, d), (d, 0, d)]:
        rc, c = _plan(_query(B, T, H, dk, ws=ws))
        assert rc == 0 and (c.path, c.dq_stored, c.ws_total) == (HEAD, dq, total)
        assert c.ws_size[L.ATTN_WS_DS] == (131072 if dq else 0)
    # the mode bit forces the recompute whatever is offered
    rc, c = _plan(_query(B, T, H, dk, ws=full, mode=M_DQ))
    assert rc == 0 and (c.dq_stored, c.ws_total) == (0, d)
    # below the path's minimum: an error naming the need, for every path
    lib = L.load()
    for kw, need in [(dict(B=B, T=T, H=H, dk=dk), d), (dict(B=1, T=385, H=1, dk=64), 1540),
                     (dict(B=2, T=130, H=2, dk=64, rel=1), 425472), (dict(B=1, T=37, H=2, dk=16, dtype=F32), 10952),
                     (dict(B=1, T=37, H=2, dk=16, dtype=F32, rel=1), 10952)]:
        assert _plan(_query(**kw, ws=need))[0] == 0
        for ws in (need - 1, 0):
            assert _plan(_query(**kw, ws=ws))[0] == -1
            assert str(need).encode() in lib.cfm_get_last_error()


def test_errors():
    lib = L.load()
    q, c = _query(2, 97, 2, 64), L.AttnChoice()
    assert lib.cfm_attn_plan(None, ctypes.byref(c)) == -1
    assert lib.cfm_attn_plan(ctypes.byref(q), None) == -1
    assert _plan(_query(2, 97, 2, 64, cus=0))[0] == -1
    for bad in (dict(B=0), dict(T=0), dict(H=-1), dict(dk=0), dict(dk=1025, dtype=F32)):
        assert _plan(_query(**dict(dict(B=2, T=97, H=2, dk=64), **bad)))[0] == -2
    assert _plan(_query(2, 97, 2, 64, dtype=L.FP8))[0] == -3
    assert _plan(_query(2, 97, 2, 128))[0] == -5                    # bf16 non-rel heads wider than 64
    assert _plan(_query(32, 16384, 8, 64))[0] == -2                 # B*H*T*(T+1) >= 2^33: the dropout index space
    assert lib.cfm_attn_bwd_ws_bytes(0, 97, 2, 64, 0, BF16) == 0
