"""The device edit distance (csrc/edit_distance.hip, ops.edit_distance, ctc.edit_distance) against the integer
restatement of tests/edit_distance_ref.py.  Every quantity is an integer: every comparison is an exact equality.

The cases (edit_distance_ref.CASES, pinned on the CPU by test_edit_distance_ref_cpu.py) are ragged batches of 1 to 7
pairs that mix references of at most 64 ids (one strip of the kernel, no LDS) with longer ones (the row carried between
strips), at the sizes around the strip width and the largest ones, over 2 symbols (ties everywhere) and 1024.
"""
import functools

import numpy as np
import pytest
import torch

from nn_conformer_for_speech_recognition_amd import _lib, ctc, ops
from tests import edit_distance_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = sorted(er.CASES)


def _pad(rows, width, fill):
    out = np.full((len(rows), width), fill, dtype=np.int64)
    for b, row in enumerate(rows):
        out[b, :len(row)] = row
    return out


def _inputs(name, extra=0, fill=0, dtype=torch.int64):
    """(hyp (B, Lh), ref (B, Lr), hyp lengths, ref lengths): the case's rows padded to the longest (+ extra columns)
    with `fill`; lengths as int64 device tensors."""
    pairs, _ = er.case(name)
    Lr = max(len(r) for r, _ in pairs) + extra
    Lh = max(len(h) for _, h in pairs) + extra
    ref = torch.from_numpy(_pad([r for r, _ in pairs], Lr, fill)).to(device=DEV, dtype=dtype)
    hyp = torch.from_numpy(_pad([h for _, h in pairs], Lh, fill)).to(device=DEV, dtype=dtype)
    rl = torch.tensor([len(r) for r, _ in pairs], device=DEV)
    hl = torch.tensor([len(h) for _, h in pairs], device=DEV)
    return hyp, ref, hl, rl


@functools.lru_cache(maxsize=None)
def _expected(name, extra=0):
    """The reference results as CPU tensors in the op's output layout (pairs padded with -1 to Lr + Lh); shared."""
    pairs, aligns = er.case(name)
    ldp = max(len(r) for r, _ in pairs) + max(len(h) for _, h in pairs) + 2 * extra
    return dict(distance=torch.tensor([a.distance for a in aligns], dtype=torch.int32),
                ref_lengths=torch.tensor([len(r) for r, _ in pairs], dtype=torch.int32),
                counts=torch.tensor([a.counts for a in aligns], dtype=torch.int32).reshape(-1, 4),
                pair_ref=torch.from_numpy(_pad([a.pair_ref for a in aligns], ldp, -1)).to(torch.int32),
                pair_hyp=torch.from_numpy(_pad([a.pair_hyp for a in aligns], ldp, -1)).to(torch.int32),
                n_pairs=torch.tensor([len(a.pair_ref) for a in aligns], dtype=torch.int32))


def _assert_equal(out, want, ops_mode=True):
    for k in ("distance", "ref_lengths") + (("counts", "pair_ref", "pair_hyp", "n_pairs") if ops_mode else ()):
        got = getattr(out, k)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want[k]), k
    if not ops_mode:
        assert out.counts is None and out.pair_ref is None and out.pair_hyp is None and out.n_pairs is None


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- the cases, both modes
@pytest.mark.parametrize("name", NAMES)
def test_cases_match_reference(name):
    hyp, ref, hl, rl = _inputs(name)
    want = _expected(name)
    plain = ctc.edit_distance(hyp, ref, hl, rl)
    full = ctc.edit_distance(hyp, ref, hl, rl, ops=True)
    _assert_equal(plain, want, ops_mode=False)
    _assert_equal(full, want)
    assert torch.equal(plain.distance, full.distance)
    c = full.counts.cpu().long()
    assert torch.equal(c[:, 0] + c[:, 1] + c[:, 2], want["ref_lengths"].long())
    assert torch.equal(c[:, 1] + c[:, 2] + c[:, 3], want["distance"].long())
    past = torch.arange(full.pair_ref.shape[1])[None, :] >= full.n_pairs.cpu()[:, None]
    assert (full.pair_ref.cpu()[past] == -1).all() and (full.pair_hyp.cpu()[past] == -1).all()


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("name", ["small_v2", "mid_v1024"])
def test_layouts_are_bit_identical(name):
    pairs, _ = er.case(name)
    want = _expected(name, extra=5)
    poison = int(pairs[-1][0][0])          # an id that occurs inside other rows
    assert any(poison in r.tolist() or poison in h.tolist() for r, h in pairs)
    hyp, ref, hl, rl = _inputs(name, extra=5, fill=poison)
    base = ctc.edit_distance(hyp, ref, hl, rl, ops=True)
    _assert_equal(base, want)
    variants = {
        "int32": (hyp.int(), ref.int(), hl.int(), rl.int()),
        "mixed": (hyp.int(), ref, hl, rl.int()),
        "host lengths": (hyp, ref, hl.tolist(), rl.tolist()),
        "cpu tensor lengths": (hyp, ref, hl.cpu(), rl.cpu()),
    }
    # rows strided inside a wider parent (row stride 2 L + 3), every other row of a taller one, both filled with poison
    for dt in (torch.int64, torch.int32):
        wide_h = torch.full((hyp.shape[0], 2 * hyp.shape[1] + 3), poison, device=DEV, dtype=dt)
        wide_r = torch.full((2 * ref.shape[0], ref.shape[1] + 1), poison, device=DEV, dtype=dt)
        wide_h[:, 2:2 + hyp.shape[1]] = hyp
        wide_r[::2, :ref.shape[1]] = ref
        hv, rv = wide_h[:, 2:2 + hyp.shape[1]], wide_r[::2, :ref.shape[1]]
        assert not hv.is_contiguous() and not rv.is_contiguous()
        variants[f"strided {dt}"] = (hv, rv, hl, rl)
    for what, args in variants.items():
        for mode in (False, True):
            out = ctc.edit_distance(*args, ops=mode)
            assert _same(out, base if mode else (base.distance, base.ref_lengths, None, None, None, None)), what


def test_none_lengths_take_the_full_row():
    pairs, _ = er.case("small_v2")
    hyp, ref, _, _ = _inputs("small_v2", fill=1)
    B, Lh, Lr = hyp.shape[0], hyp.shape[1], ref.shape[1]
    aligns = [er.align(r, h) for r, h in zip(ref.cpu().numpy(), hyp.cpu().numpy())]
    out = ctc.edit_distance(hyp, ref, ops=True)
    assert out.distance.tolist() == [a.distance for a in aligns]
    assert out.counts.tolist() == [list(a.counts) for a in aligns]
    assert out.ref_lengths.tolist() == [Lr] * B
    for b, a in enumerate(aligns):
        n = int(out.n_pairs[b])
        assert out.pair_ref[b, :n].tolist() == a.pair_ref and out.pair_hyp[b, :n].tolist() == a.pair_hyp
    for hl, rl in (([Lh] * B, [Lr] * B), (torch.full((B,), Lh, device=DEV), None), (None, torch.full((B,), Lr))):
        assert _same(ctc.edit_distance(hyp, ref, hl, rl, ops=True), out)


def test_lengths_are_clamped_to_the_row():
    """Device lengths are never read back: above the row width they count as the width, below zero as zero."""
    name = "small_v2"
    hyp, ref, hl, rl = _inputs(name)
    want = _expected(name)
    Lh, Lr = hyp.shape[1], ref.shape[1]
    hl2 = torch.where(hl == Lh, hl + 5000, torch.where(hl == 0, hl - 3, hl))
    rl2 = torch.where(rl == Lr, rl + (1 << 20), torch.where(rl == 0, rl - 1, rl))
    assert (hl2 > Lh).any() and (rl2 > Lr).any() and (hl2 < 0).any() and (rl2 < 0).any()
    _assert_equal(ctc.edit_distance(hyp, ref, hl2, rl2, ops=True), want)
    _assert_equal(ctc.edit_distance(hyp, ref, hl2, rl2), want, ops_mode=False)


# ----------------------------------------------------------------------------- guard regions
GUARD = 64
PATTERN = 0x5A5A5A5A


@pytest.mark.parametrize("name", ["small_v2", "mid_v1024", "long_v2"])
@pytest.mark.parametrize("mode", [False, True])
def test_outputs_stay_inside_their_buffers(name, mode):
    hyp, ref, hl, rl = _inputs(name, dtype=torch.int32)
    want = _expected(name)
    P, Lh, Lr = hyp.shape[0], hyp.shape[1], ref.shape[1]
    shapes = {"dist": (P,)}
    if mode:
        shapes.update(counts=(P, 4), pair_ref=(P, Lr + Lh), pair_hyp=(P, Lr + Lh), n_pairs=(P,))
    total = GUARD + sum(int(np.prod(s)) + GUARD for s in shapes.values())
    arena = torch.full((total,), PATTERN, device=DEV, dtype=torch.int32)
    out, inside, off = {}, torch.zeros(total, dtype=torch.bool), GUARD
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = arena[off:off + n].view(s)
        inside[off:off + n] = True
        off += n + GUARD
    got = ops.edit_distance(ref, ref.stride(0), rl.int(), hyp, hyp.stride(0), hl.int(), P, 1, Lr, Lh, mode, out=out)
    assert got[0].data_ptr() == out["dist"].data_ptr()
    host = arena.cpu()
    assert (host[~inside] == PATTERN).all(), "a guard region changed"
    assert torch.equal(out["dist"].cpu(), want["distance"])
    if mode:
        for k, w in (("counts", "counts"), ("pair_ref", "pair_ref"), ("pair_hyp", "pair_hyp"), ("n_pairs", "n_pairs")):
            assert torch.equal(out[k].cpu(), want[w]), k      # so also: -1 past n_pairs, no pattern left inside


# ----------------------------------------------------------------------------- n-best
def test_nbest_equals_separate_calls():
    pairs, aligns = er.case("small_v1024")
    B, N = len(pairs), 3
    hyps = [[pairs[b][1], pairs[(b + 1) % B][1], pairs[(b + 3) % B][0]] for b in range(B)]
    Lh = max(len(h) for row in hyps for h in row)
    Lr = max(len(r) for r, _ in pairs)
    hyp = torch.from_numpy(np.stack([_pad(row, Lh, 0) for row in hyps])).to(DEV)
    hl = torch.tensor([[len(h) for h in row] for row in hyps], device=DEV)
    ref = torch.from_numpy(_pad([r for r, _ in pairs], Lr, 0)).to(DEV)
    rl = torch.tensor([len(r) for r, _ in pairs], device=DEV)
    for mode in (False, True):
        out = ctc.edit_distance(hyp, ref, hl, rl, ops=mode)
        assert out.distance.shape == (B, N) and out.ref_lengths.shape == (B,)
        for n in range(N):
            one = ctc.edit_distance(hyp[:, n], ref, hl[:, n], rl, ops=mode)
            assert torch.equal(out.distance[:, n], one.distance)
            if mode:
                assert out.counts.shape == (B, N, 4) and out.pair_ref.shape == (B, N, Lr + Lh)
                assert torch.equal(out.counts[:, n], one.counts) and torch.equal(out.n_pairs[:, n], one.n_pairs)
                assert torch.equal(out.pair_ref[:, n], one.pair_ref) and torch.equal(out.pair_hyp[:, n], one.pair_hyp)
        assert out.distance[:, 0].tolist() == [a.distance for a in aligns]
        assert out.distance[:, 2].tolist() == [er.table(pairs[b][0], hyps[b][2])[-1, -1] for b in range(B)]
        assert (out.distance.min(dim=1).values <= out.distance[:, 0]).all()       # the oracle hypothesis


# ----------------------------------------------------------------------------- determinism, graphs, no sync
def test_two_runs_and_graph_replays_are_bit_identical():
    hyp, ref, hl, rl = _inputs("mid_v2")
    first = ctc.edit_distance(hyp, ref, hl, rl, ops=True)
    _assert_equal(first, _expected("mid_v2"))
    assert _same(ctc.edit_distance(hyp, ref, hl, rl, ops=True), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc.edit_distance(hyp, ref, hl, rl, ops=True)
        ctc.edit_distance(hyp, ref, hl, rl)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ctc.edit_distance(hyp, ref, hl, rl, ops=True)
        static_plain = ctc.edit_distance(hyp, ref, hl, rl)
    for _ in range(2):
        for o in tuple(static) + (static_plain.distance,):
            o.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert _same(static, first)
        assert torch.equal(static_plain.distance, first.distance)


def test_no_host_synchronisation_with_device_lengths():
    hyp, ref, hl, rl = _inputs("mid_v1024")
    ctc.edit_distance(hyp, ref, hl, rl, ops=True)          # first call: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        plain = ctc.edit_distance(hyp, ref, hl, rl)
        full = ctc.edit_distance(hyp, ref, hl, rl, ops=True)
        nbest = ctc.edit_distance(hyp[:, None, :].expand(-1, 2, -1), ref, hl[:, None].expand(-1, 2), rl)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    _assert_equal(plain, _expected("mid_v1024"), ops_mode=False)
    _assert_equal(full, _expected("mid_v1024"))
    assert torch.equal(nbest.distance[:, 1], plain.distance)


# ----------------------------------------------------------------------------- validation
def test_host_side_validation():
    ok = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ctc.edit_distance(ok, torch.zeros(2, 1025, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ctc.edit_distance(torch.zeros(2, 1025, dtype=torch.int64, device=DEV), ok)
    with pytest.raises(RuntimeError):
        ctc.edit_distance(ok.cpu(), ok)
    with pytest.raises(RuntimeError):
        ctc.edit_distance(ok, ok.cpu())
    with pytest.raises(ValueError):
        ctc.edit_distance(ok, torch.zeros(3, 8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ctc.edit_distance(ok, ok, hyp_lengths=[1, 2, 3])
    with pytest.raises(TypeError):
        ctc.edit_distance(ok.float(), ok)
    # the C entry itself: the size limit, P % group, a width above the row stride -- all before any launch
    big = torch.zeros(1, 1025, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.CfmError, match="1024"):
        ops.edit_distance(big, 1025, one, big, 1025, one, 1, 1, 1025, 8)
    ok32, three = ok.int(), torch.ones(3, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.CfmError):
        ops.edit_distance(ok32, 8, three, torch.zeros(3, 8, dtype=torch.int32, device=DEV), 8, three, 3, 2, 8, 8)
    with pytest.raises(_lib.CfmError):
        ops.edit_distance(ok32, 4, three[:2], ok32, 8, three[:2], 2, 1, 8, 8)
    assert _lib.size_call("cfm_edit_distance_ws_bytes", 32, 40, 373, 0) == 0
    assert 0 < _lib.size_call("cfm_edit_distance_ws_bytes", 32, 1024, 1024, 1) <= 32 * 1024 * (1024 + 63 + 15) // 4


# ----------------------------------------------------------------------------- through the decoders
def test_decoder_outputs_match_wer_on_strings():
    from nn_conformer_for_speech_recognition_amd.lib.standard.myvocab import Vocab, wer
    voc = Vocab(["<blank>", "<pad>"] + [f"w{i}" for i in range(10)])
    gen = torch.Generator().manual_seed(3)
    B, T, V, N = 4, 50, 12, 4
    logits = (3 * torch.randn(B, T, V, generator=gen)).to(DEV)
    tl = [9, 1, 30, 17]
    target = torch.full((B, 30), voc.pad_idx, dtype=torch.int64)
    for b, n in enumerate(tl):
        target[b, :n] = torch.randint(2, V, (n,), generator=gen)
    t_strs = voc.decode(target)
    assert [len(s.split()) for s in t_strs] == tl
    target, tld = target.to(DEV), torch.tensor(tl, device=DEV)

    _, toks, cnt = ctc.greedy_decode(logits, None, blank=voc.blank_idx, pad=voc.pad_idx, collapse=False)
    out = ctc.edit_distance(toks, target, cnt, tld)
    h_strs = voc.decode(toks, cnt)
    assert h_strs == voc.decode(torch.argmax(logits, -1))
    assert out.distance.tolist() == [round(wer(t, h) * n) for t, h, n in zip(t_strs, h_strs, tl)]

    btoks, blens, _ = ctc.beam_search_decode(logits, None, beam_size=N, blank=voc.blank_idx, pad=voc.pad_idx, nbest=N)
    out = ctc.edit_distance(btoks, target, blens, tld, ops=True)
    assert out.distance.shape == (B, N)
    for n in range(N):
        h_strs = voc.decode(btoks[:, n], blens[:, n])
        assert out.distance[:, n].tolist() == [round(wer(t, h) * k) for t, h, k in zip(t_strs, h_strs, tl)]
    c = out.counts.long()
    assert torch.equal(c[..., 1] + c[..., 2] + c[..., 3], out.distance.long())
    assert torch.equal(c[..., 0] + c[..., 1] + c[..., 3], blens.long())
