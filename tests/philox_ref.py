"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw — "Parallel random numbers: as easy as 1, 2, 3",
SC'11) in numpy, for checking the perf-mode (SD_NOISE_PHILOX) kernels.  Mirrors
csrc/sd_device.h: philox4x32_10, philox_block's counter layout, uniform_from_word,
cdf_uniform, span_gumbel, and csrc/sd_draw_nucleus.inc: nuc_uniform.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SITE_ACCEPT, SITE_SAMPLE, SITE_CDF = 1, 2, 3


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 (ints or uint64 arrays), key: 2 uint32 -> 4 uint32 (same shape)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        p0 = c0 * np.uint64(M0)
        p1 = c2 * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return c0, c1, c2, c3


def block(seed: int, offset: int, row, site: int, idx):
    ctr = (idx, (np.asarray(row, dtype=np.uint64) & np.uint64(0xFFFFFF)) | np.uint64(site << 24),
           offset & MASK, (offset >> 32) & MASK)
    return philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK))


def accept_uniform(seed: int, offset: int, row: int, i: int) -> float:
    """The accept-test uniform of draft i of row `row`: word i % 4 of block i // 4 (torch.rand's fp32
    from one word)."""
    w = int(block(seed, offset, row, SITE_ACCEPT, i >> 2)[i & 3])
    return np.float32((w & 0xFFFFFF) * 2.0 ** -24)


SITE_NUC = 4                 # k_draw_nuc's proposals (csrc/sd_draw_nucleus.inc: kSiteNuc)


def _u53(x, y):
    """U[0, 1) at 53 bits from two words, x the high one (sd_device.h cdf_uniform)."""
    v = ((np.asarray(x, dtype=np.uint64) << np.uint64(32)) | np.asarray(y, dtype=np.uint64)) >> np.uint64(11)
    return v.astype(np.float64) * 2.0 ** -53


def cdf_uniform(seed: int, offset: int, row, idx=0):
    """The inverse-CDF uniform of block (site CDF, idx) of the row: idx 0 picks the span / shard, idx 1 + c
    the element inside span c (sd_device.h cdf_uniform).  Scalars give a float; arrays of rows and / or
    indices broadcast to an fp64 array."""
    x, y, _, _ = block(seed, offset, row, SITE_CDF, idx)
    u = _u53(x, y)
    return float(u) if u.ndim == 0 else u


def span_gumbel(seed: int, offset: int, row, c):
    """k_draw_lean's span-race noise g_c = -ln E_c (sd_device.h span_gumbel): word z of block (site CDF,
    1 + c), u = (z >> 8)·2^-24 + 2^-25 in fp32 arithmetic (exp1_from_word), E = -ln u and g = -ln E in fp64
    from the fp32 u (the device takes both logarithms in fp32).  Returns (g, E): floats for scalars, fp64
    arrays otherwise."""
    z = np.asarray(block(seed, offset, row, SITE_CDF, np.asarray(c, dtype=np.uint64) + np.uint64(1))[2])
    u = (z >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    with np.errstate(divide="ignore"):
        E = -np.log(u.astype(np.float64))
        g = -np.log(E)
    return (float(g), float(E)) if g.ndim == 0 else (g, E)


def nuc_uniform(seed: int, offset: int, row, idx):
    """k_draw_nuc's 53-bit uniform of block (site 4, idx): idx = 128·(4·round + k) + (0: the row's slice
    pick | 1 + c: slice c's element pick) (sd_draw_nucleus.inc nuc_uniform)."""
    x, y, _, _ = block(seed, offset, row, SITE_NUC, idx)
    u = _u53(x, y)
    return float(u) if u.ndim == 0 else u


def exp1_words(seed: int, offset: int, row: int, site: int, n: int):
    """The perf-mode Exp(1) values of elements 0..n-1 drawn at `site` (exp1_from_word): element j reads
    word j & 3 of block j >> 2, u = (w >> 8)·2^-24 + 2^-25 in fp32 arithmetic and E = -ln u (here in
    fp64 from the fp32 u; the device takes the fp32 logarithm).  Returns (E, u) as fp64 / fp32 [n]."""
    words = np.stack(block(seed, offset, row, site, np.arange((n + 3) // 4, dtype=np.uint64)), axis=1).reshape(-1)[:n]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    with np.errstate(divide="ignore"):
        return -np.log(u.astype(np.float64)), u
