"""Host model of the multi-draft verify step (sd_verify_multi; the rule in include/specdec.h and
DESIGN.md): the walk over the prefix tree of K drafted chains by recursive rejection sampling, in
fp64 over given probability rows — the exact-arithmetic oracle's rounded probabilities
(ref.process(..., exact=True)) in the tests — and the numpy Philox (tests/philox_ref.py).

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import philox_ref as ph

MASS_TOL = 1e-5     # the project's mass tolerance, applied to each divisor the device forms in fp32
RESIDUAL, BONUS, STOP = "residual", "bonus", "stop"


class Fork(Exception):
    """Raised by an enumerating `accept` when the walk asks for a decision beyond its script."""

    def __init__(self, frac):
        self.frac = frac


def walk(P, Q, tok, accept):
    """The rule.  P [K, γ+1, V], Q [K, γ, V] fp64 arrays (row d of chain k was computed on
    prefix + tok[k, :d]); tok [K, γ] ints; accept(d, k, j, frac, slack) -> bool decides the test of
    chain k at depth d after j rejected siblings (frac = r[x] / q[x]; slack = Σ_{i<=j} 1e-5 / m_i).

    Returns a namespace: n, winner, status (RESIDUAL | BONUS), rejects, mass (of the last residual
    formed, NaN if none), weights (fp64 [V], unnormalised: the bonus row, or max(r - q, 0) of the
    last residual), final_mass (Σ weights), tests [(d, k, j, frac, accepted)], readmit (an alive set
    kept a chain that had been rejected at that depth), kept_untried (an alive set kept a same-token
    chain that had not been tested), last_slack, masses (m_1.. of the depth the
    last residual was formed at) and mass_at (its first alive chain, depth)."""
    K, g = tok.shape
    A = list(range(K))
    out = SimpleNamespace(n=g, winner=0, status=BONUS, rejects=0, mass=math.nan, weights=None, final_mass=math.nan,
                          tests=[], readmit=False, kept_untried=False, last_slack=0.0, masses=[], mass_at=None)
    with np.errstate(divide="ignore", invalid="ignore"):
        for d in range(g):
            k0 = A[0]
            q = np.asarray(Q[k0, d], dtype=np.float64)
            r = np.asarray(P[k0, d], dtype=np.float64).copy()
            hit, slack, diff, rejected = None, 0.0, None, []
            for j, k in enumerate(A):
                x = int(tok[k, d])
                inside = 0 <= x < len(r)
                frac = (r[x] / q[x]) if inside else math.nan     # 0/0 = NaN, x/0 = inf: both accept, as SPEC
                acc = bool(accept(d, k, j, float(frac), slack))
                out.tests.append((d, k, j, float(frac), acc))
                if acc:
                    hit = x
                    break
                if not rejected:
                    out.masses, out.mass_at = [], (k0, d)
                rejected.append(k)
                diff = np.maximum(r - q, 0.0)
                m = float(diff.sum())
                r = diff / m
                out.mass = m
                out.masses.append(m)
                slack += MASS_TOL / m if m > 0 else math.inf
                out.rejects += 1
                out.last_slack = slack
            if hit is None:
                out.n, out.winner, out.status = d, k0, RESIDUAL
                out.weights, out.final_mass = diff, out.mass
                return out
            A2 = [k for k in A if int(tok[k, d]) == hit]
            out.readmit |= any(k in rejected for k in A2)
            out.kept_untried |= any(k in A[len(rejected) + 1:] for k in A2)
            A = A2
    out.winner = A[0]
    out.weights = np.asarray(P[out.winner, g], dtype=np.float64)
    out.final_mass = float(out.weights.sum())
    return out


def stop_location(accepted, stops):
    """The loops' stop scan (sampling/speculative_decoding.py:150-152): the stop LISTED first that
    occurs, at its first position; -1 if none."""
    acc = [int(t) for t in accepted]
    for s in stops:
        if int(s) in acc:
            return acc.index(int(s))
    return -1


def inverse_cdf(weights, u):
    """The first index with positive weight whose running total exceeds u·Σ (the last positive one
    when rounding runs past the end)."""
    w = np.asarray(weights, dtype=np.float64)
    c = np.cumsum(w)
    pos = np.nonzero(w > 0)[0]
    over = pos[c[pos] > u * c[-1]]
    return int(over[0]) if len(over) else int(pos[-1])


def draw_interval(weights, x):
    """(lo, hi): the fp64 running total of `weights` before and after element x — the inverse CDF
    returns x for the targets u·Σ in [lo, hi)."""
    c = np.cumsum(np.asarray(weights, dtype=np.float64))
    return (float(c[x - 1]) if x > 0 else 0.0), float(c[x])


def philox_step(P, Q, tok, seed, off, row, stops=(), greedy=False):
    """One sequence's step on the Philox noise of global row `row`: walk()'s namespace plus close
    (an accept test sat within the device's fp32 tolerance of its threshold), stop_index, x (fp64
    inverse CDF on the row's cdf uniform, argmax under greedy; None on a stop exit), prune_drafter,
    prune_target, emitted (tok[winner, :n] + [x]); and of the draw: u (the row's cdf uniform), total
    (Σ weights) and lo, hi (draw_interval of x; NaN where no token was drawn by inverse CDF)."""
    K, g = tok.shape
    state = SimpleNamespace(close=False)

    def accept(d, k, j, frac, slack):
        u = float(ph.accept_uniform(seed, off, row, d * K + k))
        if frac == frac and abs(u - frac) <= (1e-6 + slack) * max(1.0, frac):
            state.close = True
        return not (u > frac)

    r = walk(P, Q, tok, accept)
    r.close = state.close
    r.accepted = [int(t) for t in tok[r.winner, :r.n]]
    r.stop_index = stop_location(r.accepted, stops)
    pruned = r.status == RESIDUAL and r.stop_index < 0
    r.prune_drafter, r.prune_target = (g - r.n, g - r.n + 1) if pruned else (0, 0)
    r.x = None
    r.u = float(ph.cdf_uniform(seed, off, row))
    r.total = float(np.sum(r.weights, dtype=np.float64))
    r.lo = r.hi = math.nan
    if r.stop_index >= 0:
        r.status = STOP
    elif greedy:
        r.x = int(np.argmax(r.weights))
    elif r.final_mass > 0:
        r.x = inverse_cdf(r.weights, r.u)
        r.lo, r.hi = draw_interval(r.weights, r.x)
    r.emitted = r.accepted + ([r.x] if r.x is not None else [])
    return r


def enumerate_outcomes(P, Q, tok):
    """Every outcome of walk() on these rows with its probability (the accept uniforms integrated
    out): a list of (probability, walk namespace).  Depth-first over scripted decisions."""
    outs = []

    def run(script, prob):
        pos = [0]

        def accept(d, k, j, frac, slack):
            if pos[0] < len(script):
                pos[0] += 1
                return script[pos[0] - 1]
            raise Fork(frac)

        try:
            outs.append((prob, walk(P, Q, tok, accept)))
        except Fork as f:
            pa = 1.0 if not f.frac < 1.0 else max(f.frac, 0.0)     # P(not u > frac), u ~ U[0, 1); NaN accepts
            if pa > 0:
                run(script + [True], prob * pa)
            if pa < 1:
                run(script + [False], prob * (1 - pa))

    run([], 1.0)
    return outs
