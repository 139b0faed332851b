"""Host model of the token-tree verify step for distinct children (sd_verify_tree_distinct; the rule
in include/specdec.h and DESIGN.md §4f): the walk from the root with exclusions, in fp64 over given
probability rows — the exact-arithmetic oracle's rounded probabilities (ref.process(..., exact=True))
in the tests — and the numpy Philox (tests/philox_ref.py).  The draw, its interval and the stop scan
are tests/multidraft_ref.py's, the topology helper tests/tree_ref.py's.

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import philox_ref as ph
from multidraft_ref import BONUS, RESIDUAL, STOP, Fork, draw_interval, inverse_cdf, stop_location  # noqa: F401
from tree_ref import children_of

CLOSE = 1e-6        # |u - ratio| <= CLOSE max(1, ratio): the device's fp32 ratio may decide the other way


def walk(P, tok, parent, accept, Y=None):
    """The rule.  P [N+1, V] fp64: the target's probabilities by slot (unnormalised: Z_s = Σ P[s]);
    tok [N] ints; accept(c, j, ratio) -> bool decides the test of node c, the j-th child of its slot
    (ratio = w / rem), asked only of a child with weight.  Y [N+1, V] (greedy): the processed logits by
    slot; a child with weight is then accepted iff Y[s][x] is the row's maximum, and `accept` is unused.

    Returns a namespace: n, path (accepted nodes), last_node, slot (where the walk ended), status
    (RESIDUAL | BONUS), rejects (children rejected), Z and rem of the exit slot, mass (rem / Z at a
    residual exit, else NaN), excluded [(token, w)] of the exit slot, weights (fp64 [V], unnormalised: the
    exit slot's row with the excluded tokens zeroed), final_mass (Σ weights) and tests
    [(c, j, ratio, accepted)] (the children with weight)."""
    ch = children_of(parent)
    out = SimpleNamespace(n=0, path=[], last_node=-1, slot=0, status=BONUS, rejects=0, mass=math.nan, weights=None,
                          final_mass=math.nan, tests=[], excluded=[], Z=math.nan, rem=math.nan, mass_at=None)
    s = 0
    while True:
        p = np.asarray(P[s], dtype=np.float64)
        Z = float(p.sum())
        rem, excluded, hit = Z, [], None
        for j, c in enumerate(ch[s]):
            x = int(tok[c])
            w = float(p[x]) if 0 <= x < len(p) and x not in [t for t, _ in excluded] else 0.0
            if w > 0:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = float(np.float64(w) / np.float64(rem))
                acc = bool(Y[s][x] == np.max(Y[s])) if Y is not None else bool(accept(c, j, ratio))
                out.tests.append((c, j, ratio, acc))
                if acc:
                    hit = c
                    break
                excluded.append((x, w))
                rem -= w
            out.rejects += 1
        if hit is None:
            break
        out.path.append(hit)
        out.last_node = hit
        s = hit + 1
    out.n, out.slot, out.Z, out.rem, out.excluded = len(out.path), s, Z, rem, excluded
    w = p.copy()
    for t, _ in excluded:
        w[t] = 0.0
    out.weights = w
    out.final_mass = float(w.sum())
    if ch[s]:
        out.status, out.mass_at = RESIDUAL, s
        with np.errstate(divide="ignore", invalid="ignore"):
            out.mass = float(np.float64(rem) / np.float64(Z))
    return out


def philox_step(P, tok, parent, seed, off, row, stops=(), Y=None):
    """One sequence's step on the Philox noise of global row `row`: walk()'s namespace plus close (an
    accept test sat within the device's fp32 tolerance of its threshold: |u - ratio| <= 1e-6 max(1,
    ratio)), stop_index, x (fp64 inverse CDF on the row's cdf uniform; under greedy — Y given — the
    argmax of the exit slot's processed logits, lowest index first; None on a stop exit or without
    mass), accepted (the path's tokens), emitted (accepted + [x]); and of the draw: u (the row's cdf
    uniform), total (Σ weights) and lo, hi (draw_interval of x; NaN where no token was drawn by
    inverse CDF)."""
    state = SimpleNamespace(close=False)

    def accept(c, j, ratio):
        u = float(ph.accept_uniform(seed, off, row, c))
        if ratio == ratio and abs(u - ratio) <= CLOSE * max(1.0, ratio):
            state.close = True
        return not (u > ratio)

    r = walk(P, tok, parent, accept, Y)
    r.close = state.close
    r.accepted = [int(tok[c]) for c in r.path]
    r.stop_index = stop_location(r.accepted, stops)
    r.x = None
    r.u = float(ph.cdf_uniform(seed, off, row))
    r.total = r.final_mass
    r.lo = r.hi = math.nan
    r.valid = bool(0 < r.Z < math.inf and 0 < r.rem < math.inf)
    if r.stop_index >= 0:
        r.status = STOP
    elif Y is not None:
        r.x = int(np.argmax(Y[r.slot]))
    elif r.valid and r.final_mass > 0:
        r.x = inverse_cdf(r.weights, r.u)
        r.lo, r.hi = draw_interval(r.weights, r.x)
    r.emitted = r.accepted + ([r.x] if r.x is not None else [])
    return r


def enumerate_outcomes(P, tok, parent):
    """Every outcome of walk() on these rows with its probability (the accept uniforms integrated
    out): a list of (probability, walk namespace).  Depth-first over scripted decisions."""
    outs = []

    def run(script, prob):
        pos = [0]

        def accept(c, j, ratio):
            if pos[0] < len(script):
                pos[0] += 1
                return script[pos[0] - 1]
            raise Fork(ratio)

        try:
            outs.append((prob, walk(P, tok, parent, accept)))
        except Fork as f:
            pa = 1.0 if not f.frac < 1.0 else max(f.frac, 0.0)     # P(not u > ratio), u ~ U[0, 1)
            if pa > 0:
                run(script + [True], prob * pa)
            if pa < 1:
                run(script + [False], prob * (1 - pa))

    run([], 1.0)
    return outs


def topk_tokens(q, k):
    """The k best indices of q: value descending, lowest index first among equals."""
    q = np.asarray(q, dtype=np.float64)
    return [int(i) for i in np.lexsort((np.arange(len(q)), -q))[:k]]
