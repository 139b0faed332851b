"""Host model of the block verify step (sd_verify_block; the rule in include/specdec.h and DESIGN.md
§4h): block verification of one drafted chain, in fp64 over given probability rows — the
exact-arithmetic oracle's rounded probabilities (ref.process(..., exact=True)) in the tests — and the
numpy Philox (tests/philox_ref.py), with the bounds the device's weights, accept probabilities and
draw are held to.

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import multidraft_ref as mref
import philox_ref as ph

RESIDUAL, BONUS, STOP = mref.RESIDUAL, mref.BONUS, mref.STOP
EPS32 = 2.0 ** -24          # half an ulp of fp32: the relative error of one rounded operation
RATIO_TOL = 1e-6            # the project's relative tolerance of a device ratio p/q (multidraft_ref.philox_step's)


# ---------------------------------------------------------------- the rule
def ratio(p, q):
    """p/q as the rule reads it: 0/0 (NaN) counts as +inf — SPEC's test accepts there."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.float64(p) / np.float64(q)
    return math.inf if a != a else float(a)


def weights(P, Q, tok):
    """w_0..w_γ: w_0 = 1, w_{t+1} = 0 if w_t == 0 else min(1, w_t P_t[x_t] / Q_t[x_t]); an id outside
    the vocabulary has p = q = 0."""
    w = [1.0]
    for t, x in enumerate(tok):
        x = int(x)
        a = ratio(P[t][x], Q[t][x]) if 0 <= x < len(P[t]) else math.inf
        w.append(0.0 if w[-1] == 0.0 else min(1.0, w[-1] * a))
    return w


def residual(P, Q, w, t):
    """max(w_t P_t - Q_t, 0), fp64 [V]."""
    return np.maximum(w[t] * np.asarray(P[t], dtype=np.float64) - np.asarray(Q[t], dtype=np.float64), 0.0)


def accept_prob(S, w):
    """h = S / (S + 1 - w); a divisor <= 0 gives 0."""
    div = S + 1.0 - w
    return 0.0 if div <= 0 else S / div


def rule(P, Q, tok):
    """(w [γ+1], S [γ], h [γ+1]) of one sequence; h[0] is unused (NaN), h[γ] = w[γ]."""
    g = len(tok)
    w = weights(P, Q, tok)
    S = [float(residual(P, Q, w, t).sum()) for t in range(g)]
    h = [math.nan] + [accept_prob(S[t], w[t]) for t in range(1, g)] + [w[g]]
    return w, S, h


def walk(P, Q, tok, accept):
    """The rule.  P [γ+1, V], Q [γ, V] fp64 arrays; tok [γ] ints; accept(t, h) -> bool decides the test
    of depth t (asked from t = γ downwards: the largest passing depth wins, so the first yes ends it).

    Returns a namespace: n, status (RESIDUAL | BONUS), w, S, h, mass (S_n, NaN on a bonus exit), weights
    (fp64 [V], unnormalised: the bonus row or max(w_n P_n - Q_n, 0)), final_mass (Σ weights)."""
    g = len(tok)
    w, S, h = rule(P, Q, tok)
    n = 0
    for t in range(g, 0, -1):
        if accept(t, h[t]):
            n = t
            break
    out = SimpleNamespace(n=n, w=w, S=S, h=h)
    if n == g:
        out.status, out.mass = BONUS, math.nan
        out.weights = np.asarray(P[g], dtype=np.float64)
    else:
        out.status, out.mass = RESIDUAL, S[n]
        out.weights = residual(P, Q, w, n)
    out.final_mass = float(out.weights.sum())
    return out


def tokenwise_n(P, Q, tok, uniforms):
    """n of the token-wise SPEC walk on the same rows, drafts and accept uniforms."""
    for t, x in enumerate(tok):
        x = int(x)
        a = ratio(P[t][x], Q[t][x]) if 0 <= x < len(P[t]) else math.inf
        if uniforms[t] > a:
            return t
    return len(tok)


def enumerate_outcomes(P, Q, tok):
    """Every outcome of walk() on these rows with its probability (the accept uniforms integrated out;
    they are independent U[0, 1)): a list of (probability, walk namespace)."""
    outs = []

    def run(script, prob):
        pos = [0]

        def accept(t, h):
            if pos[0] < len(script):
                pos[0] += 1
                return script[pos[0] - 1]
            raise mref.Fork(h)

        try:
            outs.append((prob, walk(P, Q, tok, accept)))
        except mref.Fork as f:
            pa = min(max(f.frac, 0.0), 1.0)          # P(not u > h), u ~ U[0, 1)
            if pa > 0:
                run(script + [True], prob * pa)
            if pa < 1:
                run(script + [False], prob * (1 - pa))

    run([], 1.0)
    return outs


def tokenwise_expectation(P, Q, tok):
    """E[n] of the token-wise walk on these rows and drafts: Σ_t Π_{s<t} min(1, a_s)."""
    e, run = 0.0, 1.0
    for t, x in enumerate(tok):
        run *= min(1.0, ratio(P[t][int(x)], Q[t][int(x)]))
        e += run
    return e


def context_free_expectations(p, q, g):
    """(block E[n], token-wise E[n], block E[n²]) with every row pair (p, q), the bonus row p, drafts
    iid from q: exact, by enumeration over the V^γ drafts and the outcomes of each."""
    import itertools
    V = len(p)
    P, Q = np.array([p] * (g + 1)), np.array([q] * g)
    qn = np.asarray(q, dtype=np.float64) / np.sum(q)
    eb = et = eb2 = 0.0
    for tok in itertools.product(range(V), repeat=g):
        pr = float(np.prod([qn[x] for x in tok]))
        if pr == 0:
            continue
        for po, o in enumerate_outcomes(P, Q, tok):
            eb += pr * po * o.n
            eb2 += pr * po * o.n * o.n
        et += pr * tokenwise_expectation(P, Q, tok)
    return eb, et, eb2


# ---------------------------------------------------------------- the device's error bounds
def weight_bound(t):
    """|device w_t - host w_t|: w_t is a product of t ratios clipped at 1, each ratio within RATIO_TOL
    (relative) of the host's and rounded once, each product rounded once; min(1, .) is 1-Lipschitz and
    w <= 1, so the relative errors add up to first order."""
    return t * (RATIO_TOL + 2 * EPS32)


def mass_bound(s_tol, t):
    """|device S_t - host S_t|: the mass tolerance of the row pair at the host's own weight (s_tol:
    multidraft_ref.MASS_TOL plus multi_walk.flip_slack of the two rows) plus what the weight's error
    moves the sum by — |∂S/∂w| = Σ_{w p > q} p <= Σ p <= 1 + flip — with the fp32 rounding of each
    fmaf(w, p, -q) within flip_slack's per-element allowance."""
    return s_tol + weight_bound(t) * (1.0 + s_tol)


def accept_bounds(S, w, t, g, s_tol):
    """(lo, hi) the device's h_t lies in: h = S / (S + 1 - w) rises with S and with w, so the corners
    (S -+ mass_bound, w -+ weight_bound), clipped to S >= 0 and 0 <= w <= 1, bound it; one more fp32
    rounding for the result.  t = γ: h = w_γ."""
    dw = weight_bound(t)
    if t == g:
        return max(w - dw, 0.0), min(w + dw, 1.0)
    dS = mass_bound(s_tol, t)
    lo = accept_prob(max(S - dS, 0.0), max(w - dw, 0.0))
    hi = accept_prob(S + dS, min(w + dw, 1.0))
    if S - dS <= 0 and w + dw >= 1:                  # the divisor may vanish: 0/0 -> 0, or S/S = 1
        lo, hi = 0.0, 1.0
    return lo * (1 - 2 * EPS32), hi * (1 + 2 * EPS32)


def philox_step(P, Q, tok, seed, off, row, stops=(), greedy=False, s_tol=None, bonus_tol=mref.MASS_TOL):
    """One sequence's step on the Philox noise of global row `row`: walk()'s namespace plus uniforms,
    tokenwise_n, rescue (n above the token-wise walk's on the same uniforms), h_lo / h_hi (accept_bounds
    per depth), close, stop_index, x (fp64 inverse CDF on the row's cdf uniform, argmax under greedy;
    None on a stop exit), prune_drafter, prune_target, emitted, and of the draw: u, total, lo, hi,
    draw_slack.  s_tol [γ]: the row pairs' mass tolerances (default MASS_TOL); bonus_tol: the bonus row's.

    close: some |u_t - h_t| lies within the decision's error bound (the device may decide that depth
    the other way), or the draw's target u·Σ lies within draw_slack of an end of the token's interval."""
    g = len(tok)
    s_tol = [mref.MASS_TOL] * g if s_tol is None else list(s_tol)
    uni = [float(ph.accept_uniform(seed, off, row, i)) for i in range(g)]
    r = walk(P, Q, tok, lambda t, h: not (uni[t - 1] > h))
    r.uniforms = uni
    r.tokenwise_n = tokenwise_n(P, Q, tok, uni)
    r.rescue = r.n > r.tokenwise_n
    r.h_lo, r.h_hi = [math.nan] * (g + 1), [math.nan] * (g + 1)
    r.close = False
    for t in range(1, g + 1):
        r.h_lo[t], r.h_hi[t] = accept_bounds(r.S[t] if t < g else 0.0, r.w[t], t, g, s_tol[t] if t < g else 0.0)
        if r.h_lo[t] <= uni[t - 1] <= r.h_hi[t]:
            r.close = True
    r.accepted = [int(t) for t in tok[:r.n]]
    r.stop_index = mref.stop_location(r.accepted, stops)
    pruned = r.status == RESIDUAL and r.stop_index < 0
    r.prune_drafter, r.prune_target = (g - r.n, g - r.n + 1) if pruned else (0, 0)
    r.x = None
    r.u = float(ph.cdf_uniform(seed, off, row))
    r.total = float(np.sum(r.weights, dtype=np.float64))
    r.lo = r.hi = math.nan
    r.draw_slack = bonus_tol if r.status == BONUS else mass_bound(s_tol[r.n], r.n)
    if r.stop_index >= 0:
        r.status = STOP
    elif greedy:
        r.x = int(np.argmax(r.weights))
    elif r.final_mass > 0:
        r.x = mref.inverse_cdf(r.weights, r.u)
        r.lo, r.hi = mref.draw_interval(r.weights, r.x)
        t = r.u * r.total
        if min(t - r.lo, r.hi - t) <= r.draw_slack:
            r.close = True
    r.emitted = r.accepted + ([r.x] if r.x is not None else [])
    return r
