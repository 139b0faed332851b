"""Host model of the vocabulary-parallel verify step (sd_vp_stats / sd_vp_decide / sd_vp_finish; the
rule in include/specdec.h and DESIGN.md §4d), in fp64 over given probability rows — the
exact-arithmetic oracle's rounded probabilities of the WHOLE rows (ref.process(..., exact=True)) in
the tests — and the numpy Philox (tests/philox_ref.py).

The walk is the multi-draft host model at K = 1 (tests/multidraft_ref.py: n, status, stop index, prune
lengths, the weights w and `close`); on top of it come the per-slice masses M_s = Σ_{j in slice} w_j,
the shard pick on u1 = cdf uniform idx 0 of the row and the in-slice inverse CDF on u2 = cdf uniform
idx 1.  γ' = 0 is "sample the one target row".

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import multidraft_ref as mref
import philox_ref as ph

MASS_TOL = mref.MASS_TOL


cdf_uniform = ph.cdf_uniform     # (seed, off, row, idx): the one definition, tests/philox_ref.py


def bounds(sizes):
    """[(offset, size)] of a partition given its slice sizes."""
    out, at = [], 0
    for n in sizes:
        out.append((at, int(n)))
        at += int(n)
    return out


def even_sizes(world: int, vocab: int):
    q, r = divmod(vocab, world)
    return [q + (1 if s < r else 0) for s in range(world)]


def pick(weights, sizes, u1: float, u2: float, greedy: bool = False):
    """The two-level draw over weights w [V] split into slices: namespace of masses [S], M, owner,
    x, prefix (the owner's interval [lo, hi) of the shard prefix sums) and inner (the token's
    interval of the in-slice prefix sums); owner = x = None when nothing can be drawn."""
    w = np.asarray(weights, dtype=np.float64)
    bs = bounds(sizes)
    assert bs[-1][0] + bs[-1][1] == len(w)
    masses = np.array([w[o:o + n].sum() for o, n in bs])
    out = SimpleNamespace(masses=masses, M=float(masses.sum()), owner=None, x=None, prefix=None, inner=None)
    if greedy:
        out.x = int(np.argmax(w))                      # lowest index among equal maxima
        out.owner = next(s for s, (o, n) in enumerate(bs) if o <= out.x < o + n)
        return out
    if not (out.M > 0 and math.isfinite(out.M)):
        return out
    cum = np.cumsum(masses)
    pos = np.nonzero(masses > 0)[0]
    over = pos[cum[pos] > u1 * out.M]
    out.owner = int(over[0]) if len(over) else int(pos[-1])
    out.prefix = (float(cum[out.owner] - masses[out.owner]), float(cum[out.owner]))
    o, n = bs[out.owner]
    j = mref.inverse_cdf(w[o:o + n], u2)
    out.x = o + j
    c = np.cumsum(w[o:o + n])
    out.inner = (float(c[j] - w[o + j]), float(c[j]))
    return out


def intervals(weights, sizes):
    """(shard prefix intervals [S, 2], per-token in-slice intervals [V, 2]) of the two-level draw."""
    w = np.asarray(weights, dtype=np.float64)
    bs = bounds(sizes)
    masses = np.array([w[o:o + n].sum() for o, n in bs])
    cum = np.cumsum(masses)
    shard_iv = np.stack([cum - masses, cum], axis=1)
    tok_iv = np.zeros((len(w), 2))
    for o, n in bs:
        c = np.cumsum(w[o:o + n])
        tok_iv[o:o + n, 0], tok_iv[o:o + n, 1] = c - w[o:o + n], c
    return shard_iv, tok_iv


def step(P, Q, tok, seed: int, off: int, row: int, sizes, stops=(), greedy: bool = False, skip: bool = False):
    """One sequence's vocabulary-parallel step.  P [γ+1, V], Q [γ, V] fp64 (whole rows), tok [γ];
    sizes: the slice sizes.  Returns multidraft_ref.philox_step's namespace at K = 1 (n, status,
    stop_index, prune_drafter, prune_target, weights, close, ...) plus resample_mass (the walk's mass
    when a residual was formed, else NaN), u1, u2 and pick()'s fields (masses, M, owner, x, prefix,
    inner; x replaces the single-uniform draw)."""
    P = np.asarray(P, dtype=np.float64)
    g = len(tok)
    Q = np.asarray(Q, dtype=np.float64).reshape(g, P.shape[-1])
    r = mref.philox_step(P[None], Q[None], np.asarray(tok, dtype=np.int64).reshape(1, g), seed, off, row, stops,
                         greedy=greedy)
    if skip and r.status == mref.RESIDUAL:                 # sample p_n itself (skip_sample_adjustment)
        r.weights = P[r.n]
        r.final_mass = float(r.weights.sum())
    r.resample_mass = r.mass if (r.status == mref.RESIDUAL and not skip) else math.nan
    r.u1, r.u2 = cdf_uniform(seed, off, row, 0), cdf_uniform(seed, off, row, 1)
    r.sizes = list(sizes)
    if r.status == mref.STOP:
        r.masses, r.M, r.owner, r.x, r.prefix, r.inner = None, math.nan, None, None, None, None
        return r
    p = pick(r.weights, sizes, r.u1, r.u2, greedy)
    r.masses, r.M, r.owner, r.x, r.prefix, r.inner = p.masses, p.M, p.owner, p.x, p.prefix, p.inner
    r.emitted = r.accepted + ([r.x] if r.x is not None else [])
    return r
