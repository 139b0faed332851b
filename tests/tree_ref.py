"""Host model of the token-tree verify step (sd_verify_tree; the rule in include/specdec.h and
DESIGN.md §4e): the walk from the root by recursive rejection sampling, in fp64 over given
probability rows — the exact-arithmetic oracle's rounded probabilities
(ref.process(..., exact=True)) in the tests — and the numpy Philox (tests/philox_ref.py).  The draw,
its interval and the stop scan are tests/multidraft_ref.py's.

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import philox_ref as ph
from multidraft_ref import (BONUS, MASS_TOL, RESIDUAL, STOP, Fork, draw_interval, inverse_cdf,  # noqa: F401
                            stop_location)


def children_of(parent):
    """children[s] of every slot s (slot 0 the root, slot i+1 node i), ascending node index."""
    ch = [[] for _ in range(len(parent) + 1)]
    for i, p in enumerate(parent):
        ch[int(p) + 1].append(i)
    return ch


def walk(P, Q, tok, parent, accept):
    """The rule.  P [N+1, V] fp64: the target's probabilities by slot; Q [N+1, V] (or a sequence with
    None at leaf slots): the drafter's, read at internal slots only; tok [N] ints; accept(c, j, frac,
    slack) -> bool decides the test of node c after j rejected siblings (frac = r[x] / q[x];
    slack = Σ_{i<=j} 1e-5 / m_i).

    Returns a namespace: n, path (accepted nodes), last_node, slot (where the walk ended), status
    (RESIDUAL | BONUS), rejects, mass (of the last residual formed, NaN if none), weights (fp64 [V],
    unnormalised: the leaf's target row, or max(r - q, 0) of the last residual), final_mass
    (Σ weights), tests [(c, j, frac, accepted)], last_slack, masses (m_1.. of the slot the last
    residual was formed at) and mass_at (that slot)."""
    ch = children_of(parent)
    out = SimpleNamespace(n=0, path=[], last_node=-1, slot=0, status=BONUS, rejects=0, mass=math.nan, weights=None,
                          final_mass=math.nan, tests=[], last_slack=0.0, masses=[], mass_at=None)
    s = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while ch[s]:
            q = np.asarray(Q[s], dtype=np.float64)
            r = np.asarray(P[s], dtype=np.float64).copy()
            hit, slack, diff, first = None, 0.0, None, True
            for j, c in enumerate(ch[s]):
                x = int(tok[c])
                inside = 0 <= x < len(r)
                frac = (r[x] / q[x]) if inside else math.nan     # 0/0 = NaN, x/0 = inf: both accept, as SPEC
                acc = bool(accept(c, j, float(frac), slack))
                out.tests.append((c, j, float(frac), acc))
                if acc:
                    hit = c
                    break
                if first:
                    out.masses, out.mass_at, first = [], s, False
                diff = np.maximum(r - q, 0.0)
                m = float(diff.sum())
                r = diff / m
                out.mass = m
                out.masses.append(m)
                slack += MASS_TOL / m if m > 0 else math.inf
                out.rejects += 1
                out.last_slack = slack
            if hit is None:
                out.slot, out.status = s, RESIDUAL
                out.weights, out.final_mass = diff, out.mass
                out.n = len(out.path)
                return out
            out.path.append(hit)
            out.last_node = hit
            s = hit + 1
    out.n, out.slot = len(out.path), s
    out.weights = np.asarray(P[s], dtype=np.float64)
    out.final_mass = float(out.weights.sum())
    return out


def philox_step(P, Q, tok, parent, seed, off, row, stops=(), greedy=False):
    """One sequence's step on the Philox noise of global row `row`: walk()'s namespace plus close
    (an accept test sat within the device's fp32 tolerance of its threshold:
    |u - ratio| <= (1e-6 + Σ 1e-5 / m_i) max(1, ratio)), stop_index, x (fp64 inverse CDF on the row's
    cdf uniform, argmax under greedy; None on a stop exit), accepted (the path's tokens), emitted
    (accepted + [x]); and of the draw: u (the row's cdf uniform), total (Σ weights) and lo, hi
    (draw_interval of x; NaN where no token was drawn by inverse CDF)."""
    state = SimpleNamespace(close=False)

    def accept(c, j, frac, slack):
        u = float(ph.accept_uniform(seed, off, row, c))
        if frac == frac and abs(u - frac) <= (1e-6 + slack) * max(1.0, frac):
            state.close = True
        return not (u > frac)

    r = walk(P, Q, tok, parent, accept)
    r.close = state.close
    r.accepted = [int(tok[c]) for c in r.path]
    r.stop_index = stop_location(r.accepted, stops)
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


def enumerate_outcomes(P, Q, tok, parent):
    """Every outcome of walk() on these rows with its probability (the accept uniforms integrated
    out): a list of (probability, walk namespace).  Depth-first over scripted decisions."""
    outs = []

    def run(script, prob):
        pos = [0]

        def accept(c, j, frac, slack):
            if pos[0] < len(script):
                pos[0] += 1
                return script[pos[0] - 1]
            raise Fork(frac)

        try:
            outs.append((prob, walk(P, Q, tok, parent, accept)))
        except Fork as f:
            pa = 1.0 if not f.frac < 1.0 else max(f.frac, 0.0)     # P(not u > frac), u ~ U[0, 1); NaN accepts
            if pa > 0:
                run(script + [True], prob * pa)
            if pa < 1:
                run(script + [False], prob * (1 - pa))

    run([], 1.0)
    return outs


def chains_rows(P, Q):
    """The slot rows of the K-chains tree (node d*K + k) from multidraft_ref's P [K, γ+1, V],
    Q [K, γ, V]: slot 0 takes chain 0's depth-0 rows (every chain's are the same rows there), the slot
    of node d*K + k chain k's rows of depth d + 1."""
    K, g1, V = P.shape
    g = g1 - 1
    Pt, Qt = np.zeros((K * g + 1, V)), np.zeros((K * g + 1, V))
    Pt[0], Qt[0] = P[0, 0], Q[0, 0]
    for d in range(g):
        for k in range(K):
            Pt[d * K + k + 1] = P[k, d + 1]
            if d + 1 < g:
                Qt[d * K + k + 1] = Q[k, d + 1]
    return Pt, Qt
