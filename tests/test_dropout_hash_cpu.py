"""Checks of the dropout element hash (cfm_common.h attn_mix: two 24-bit multiply-adds), which every dropout of the
library uses (attention probabilities, GEMM epilogues, scale_dropout, the LayerNorm backward's g2; lowbias32 =
cfm_mix32 only derives the per-call key):
* it is one-to-one on 32 bits (2^25 consecutive pair indices under a random key all hash apart; x and
  x ^ (d * 0x01000100), the collision class of round 4's form, never collide);
* keep rate and keep-decision correlations at lags 1..8 along both axes and both diagonals, next to lowbias32 as
  the reference quality, over the attention index pattern ((b H + h) T + i) T2 + j/2 (+ key) and over the GEMM
  epilogue layout doff + (z M + m) N + n at the L15 FFN-up size (M 11,936, N 2048).  numpy only (CPU)."""
import numpy as np
import pytest

from tests import dropout_hash as dh
from tests.dropout_hash import M, attn_mix, mix32


def _lowbias32_keyed(x, key):
    return mix32((x ^ np.uint64(key)) & M)


def _attn_keyed(x, key):
    return attn_mix((x + np.uint64(key)) & M)


def _halves(h, thr):
    return np.stack([(h & 0xFFFF) >= thr, (h >> 16) >= thr], -1)


def _keep_attn(f, nbh, T, key, p=0.1):
    T2 = (T + 1) // 2
    thr = int(p * 65536 + 0.5)
    bh = np.arange(nbh, dtype=np.uint64)[:, None, None]
    i = np.arange(T, dtype=np.uint64)[None, :, None]
    jp = np.arange(T2, dtype=np.uint64)[None, None, :]
    h = f((bh * T + i) * T2 + jp, key)
    return _halves(h, thr).reshape(nbh, T, 2 * T2)[:, :, :T].astype(np.float32)


def _keep_gemm(f, Mrows, N, doff, key, p=0.1):
    """the GEMM epilogue's keep mask of an (Mrows, N) output: element e = doff + m N + n, pair e / 2 (N even, doff
    even, so each pair is two neighbouring columns of one row)."""
    thr = int(p * 65536 + 0.5)
    m = np.arange(Mrows, dtype=np.uint64)[:, None]
    jp = np.arange(N // 2, dtype=np.uint64)[None, :]
    h = f((doff // 2 + m * (N // 2) + jp) & M, key)
    return _halves(h, thr).reshape(1, Mrows, N).astype(np.float32)


def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def _worst_corr(k):
    w = 0.0
    for lag in range(1, 9):
        w = max(w, abs(_corr(k[:, :, :-lag], k[:, :, lag:])), abs(_corr(k[:, :-lag, :], k[:, lag:, :])))
    w = max(w, abs(_corr(k[:, :-1, :-1], k[:, 1:, 1:])), abs(_corr(k[:, :-1, 1:], k[:, 1:, :-1])))
    return w


def _check(k, ref, row_len):
    n = k.size
    assert abs(k.mean() - 0.9) < 4 * np.sqrt(0.09 / n)           # keep rate 1 - p within 4 sigma
    noise = 5.0 / np.sqrt(n)
    assert _worst_corr(k) < max(noise, 1.5 * _worst_corr(ref))  # no structure beyond lowbias32's / noise
    rows = k.mean(axis=2)                                         # per-row keep rates ~ binomial
    assert rows.std() < 1.25 * np.sqrt(0.09 / row_len)


@pytest.mark.parametrize("T,nbh", [(373, 16), (1498, 4)])
def test_attn_mix_keep_statistics(T, nbh):
    rng = np.random.default_rng(T)
    for key in rng.integers(0, 2 ** 32, 2, dtype=np.uint64):
        _check(_keep_attn(_attn_keyed, nbh, T, key), _keep_attn(_lowbias32_keyed, nbh, T, key), T)


def test_gemm_epilogue_keep_statistics():
    """the FFN-up epilogue's dropout at L15 (M 11,936 rows, N 2048): 24.4 M elements, 12.2 M pairs."""
    rng = np.random.default_rng(2048)
    key = rng.integers(0, 2 ** 32, dtype=np.uint64)
    doff = 2 * int(rng.integers(0, 2 ** 20))
    _check(_keep_gemm(_attn_keyed, 11936, 2048, doff, key), _keep_gemm(_lowbias32_keyed, 11936, 2048, doff, key), 2048)


def test_attn_mix_is_one_to_one():
    rng = np.random.default_rng(5)
    key = np.uint64(rng.integers(0, 2 ** 32, dtype=np.uint64))
    h = attn_mix((np.arange(1 << 25, dtype=np.uint64) + key) & M).astype(np.uint32)
    assert np.unique(h).size == h.size                           # 2^25 pair indices, all distinct
    x = rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64)
    hx = attn_mix(x)
    for d in range(1, 256):                                      # round 4's collision class
        assert not np.any(attn_mix(x ^ np.uint64(d * 0x01000100)) == hx)
    # each round x + lo24(x) * C is a bijection: 2^16 random lo24 values under all 256 high bytes stay distinct
    lo = rng.integers(0, 1 << 24, 1 << 16, dtype=np.uint64)
    lo = np.unique(lo)[:, None]
    w = lo + (np.arange(256, dtype=np.uint64)[None, :] << np.uint64(24))
    for C in (0x9E3778, 0x85EBCA):
        r = (w + (w & 0xFFFFFF) * C) & M
        assert np.unique(r.astype(np.uint32)).size == r.size


# ------------------------------------------------------------------------------------ the mask helpers
SEEDS = [5, (1 << 40) + 5, dh.salted(5, 3)]


def _drop_bits_scalar(seed, idx):
    """drop_bits of cfm_common.h, one element at a time on Python integers (no numpy: a second transcription)"""
    def mix(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M
        x ^= x >> 15
        x = (x * 0x846CA68B) & M
        return x ^ (x >> 16)

    def amix(x):
        x ^= x >> 16
        x = (x + (x & 0xFFFFFF) * 0x9E3778) & M
        x ^= x >> 15
        x = (x + (x & 0xFFFFFF) * 0x85EBCA) & M
        return x ^ (x >> 16)
    j = idx >> 1
    key = mix((j >> 32) ^ (seed & M) ^ mix(((seed >> 32) + 0x9E3779B9) & M))
    h = amix(((j & M) + key) & M)
    return h >> 16 if idx & 1 else h & 0xFFFF


@pytest.mark.parametrize("seed", SEEDS)
def test_flat_keep_matches_the_scalar_transcription_and_its_offset_is_a_shift(seed):
    p, n = 0.1, 1003
    full = dh.flat_keep(n, p, seed)
    assert full.dtype == np.bool_ and full.shape == (n,)
    thr = dh.drop_thr(p)
    assert thr == 6554
    for i in list(range(40)) + [n - 1]:
        assert bool(full[i]) == (_drop_bits_scalar(seed, i) >= thr)
    for o in (1, 3, 8):       # an odd offset moves every element to the other half of its pair hash
        np.testing.assert_array_equal(dh.flat_keep(n - o, p, seed, offset=o), full[o:])
    np.testing.assert_array_equal(dh.flat_keep((17, 59), p, seed), full.reshape(17, 59))


def test_wide_and_salted_seeds_differ_from_their_low_words():
    p, n = 0.1, 385 * 77
    wide = (1 << 40) + 5
    assert wide & M == 5
    assert (dh.flat_keep(n, p, wide) != dh.flat_keep(n, p, 5)).mean() > 0.1       # independent masks: 2 p (1 - p)
    s = dh.salted(5, 3)
    assert s == (5 + 3 * 0x9E3779B97F4A7C15) - (1 << 64) and s >> 32 != 0         # 64-bit wrap-around, as the device
    assert dh.salted(5, 0) == 5 and dh.salted(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert (dh.flat_keep(n, p, s) != dh.flat_keep(n, p, s & M)).mean() > 0.1
    assert (dh.flat_keep(n, p, s) != dh.flat_keep(n, p, 5)).mean() > 0.1


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_rate_is_the_thresholds(seed):
    """385 x 77 = 29,645 elements: the keep rate within 4 binomial sigma of 1 - thr / 65536 (sigma 0.0017 at p 0.1)"""
    p, n = 0.1, 385 * 77
    q = 1 - dh.drop_thr(p) / 65536
    rate = dh.gemm_keep(385, 77, p, seed).mean()
    assert abs(rate - q) < 4 * np.sqrt(q * (1 - q) / n), rate
    assert dh.keep_scale(p) == 65536 / (65536 - 6554) and abs(dh.keep_scale(p) - 1 / q) < 1e-12
    assert abs(dh.keep_scale(p) - 1 / 0.9) > 1e-6          # not 1 / (1 - p): the threshold is an integer
    assert dh.keep_scale(0.5) == 2.0


def test_gemm_and_attention_index_conventions():
    p, seed = 0.1, 77
    Mr, N = 37, 77
    flat = dh.flat_keep(3 + 2 * Mr * N, p, seed)
    g = dh.gemm_keep(Mr, N, p, seed, offset=3, batch=2)
    assert g.shape == (2, Mr, N)
    np.testing.assert_array_equal(g.reshape(-1), flat[3:])               # z M N + m N + n, behind the offset
    np.testing.assert_array_equal(dh.gemm_keep(Mr, N, p, seed), flat[:Mr * N].reshape(Mr, N))
    B, H = 2, 2
    for T in (6, 7):                                                      # rows of the even stride T + (T & 1)
        Te = T + (T & 1)
        a = dh.attn_keep(B, H, T, p, seed)
        assert a.shape == (B, H, T, T)
        rows = dh.flat_keep((B * H * T, Te), p, seed)
        np.testing.assert_array_equal(a.reshape(B * H * T, T), rows[:, :T])
