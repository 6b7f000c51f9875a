"""numpy restatement of the device dropout hash (test infrastructure; cfm_common.h cfm_mix32 / attn_mix / drop_key /
drop_bits).  Element idx of a call keyed by `seed` keeps iff the 16-bit half (idx & 1) of attn_mix(idx/2 + key) is
>= round(p * 65536).

The mask helpers below restate the index convention of each dropout site from its documentation (cfm_common.h:
drop_bits / drop_thr / drop_keep_scale / salted_seed; attn_common.h: didx; gemm_epilogue.h: the element index of an
epilogue), never by calling the library:
* flat_keep   element i of a flat call (cfm_scale_dropout, the LayerNorm backward's g2): index offset + i;
* gemm_keep   element (z, m, n) of a GEMM epilogue: index offset + z M N + m N + n (the output's LOGICAL position, not
              its ldc-strided address);
* attn_keep   attention probability (b, h, i, j): index ((b H + h) T + i) T_even + j, T_even = T rounded up to even;
* salted      the seed a kernel uses while a device step counter is bound (cfm_rng_bind)."""
import numpy as np

M = 0xFFFFFFFF


def mix32(x):
    """lowbias32 (cfm_mix32): derives the per-call key."""
    x = np.asarray(x).astype(np.uint64) & M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def attn_mix(x):
    """the element hash: two rounds x += lo24(x) * C (C even) -- a bijection of the 32-bit word."""
    x = np.asarray(x).astype(np.uint64) & M
    x ^= x >> 16
    x = (x + (x & 0xFFFFFF) * 0x9E3778) & M
    x ^= x >> 15
    x = (x + (x & 0xFFFFFF) * 0x85EBCA) & M
    x ^= x >> 16
    return x


def drop_key(seed, jhi=0):
    inner = int(mix32(np.array([((seed >> 32) + 0x9E3779B9) & M]))[0])
    return int(mix32(np.array([(jhi ^ (seed & M) ^ inner) & M]))[0])


def drop_thr(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_bits(idx, key):
    """16 uniform bits of element idx (idx < 2^33, where drop_key's high word is 0)."""
    idx = np.asarray(idx).astype(np.uint64)
    h = attn_mix(((idx >> 1) + np.uint64(key)) & M)
    return np.where(idx & 1, h >> 16, h & 0xFFFF)


def keep_scale(p):
    """what a kept element is multiplied by (drop_keep_scale): the exact inverse of the keep probability the integer
    threshold realises, 65536 / (65536 - thr) -- not 1 / (1 - p).  A Python float (the device rounds it to fp32)."""
    return 65536.0 / (65536 - drop_thr(p))


def salted(seed, counter):
    """salted_seed: the seed a kernel uses while a device step counter of value `counter` is bound."""
    return (int(seed) + int(counter) * 0x9E3779B97F4A7C15) % (1 << 64)


def flat_keep(n_or_shape, p, seed, offset=0):
    """bool keep mask of a flat call's elements offset + 0 .. offset + n - 1, in the given shape (row-major)."""
    shape = (int(n_or_shape),) if np.isscalar(n_or_shape) else tuple(int(s) for s in n_or_shape)
    n = int(np.prod(shape, dtype=np.int64))
    idx = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    assert n == 0 or int(idx[-1]) < 1 << 33
    return (keep_bits(idx, drop_key(seed)) >= drop_thr(p)).reshape(shape)


def gemm_keep(M_rows, N, p, seed, offset=0, batch=1):
    """bool keep mask of a GEMM epilogue's (batch, M, N) output -- (M, N) for batch 1: element offset + z M N + m N + n."""
    z = np.arange(batch, dtype=np.uint64)[:, None, None]
    m = np.arange(M_rows, dtype=np.uint64)[None, :, None]
    n = np.arange(N, dtype=np.uint64)[None, None, :]
    idx = np.uint64(offset) + z * np.uint64(M_rows * N) + m * np.uint64(N) + n
    assert int(idx.max(initial=0)) < 1 << 33
    keep = keep_bits(idx, drop_key(seed)) >= drop_thr(p)
    return keep[0] if batch == 1 else keep


def attn_keep(B, H, T, p, seed):
    """numpy restatement of the attention-dropout keep mask (cfm_common.h attn_mix / drop_key, attn_common.h
    didx): element (b, h, i, j) keeps iff the 16-bit half (j & 1) of attn_mix(((bh T + i) T2 + j/2) + key) >= thr,
    T2 = (T rounded up to even) / 2, key = lowbias32-derived drop_key(seed, 0).  Returns (B, H, T, T) bool."""
    key = drop_key(seed)
    thr = drop_thr(p)
    T2 = (T + (T & 1)) >> 1
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(T, dtype=np.uint64)[None, :, None]
    j = np.arange(T, dtype=np.uint64)[None, None, :]
    hs = attn_mix((((bh * T + i) * T2 + j // 2) + key) & 0xFFFFFFFF)
    half = np.where(j % 2 == 0, hs & 0xFFFF, hs >> 16)
    return (half >= thr).reshape(B, H, T, T)
