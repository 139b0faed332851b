"""Host models of the without-replacement token trees: sd_sample_distinct's Gumbel top-k in fp64 on
the same Philox words, sd_verify_tree_swor's walk in fp64 (tests/tree_ref.py's namespace, so tests/tree_walk.py's
bounds apply) and the exact enumeration of draw and walk together.  No GPU, no library import."""
from __future__ import annotations

import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

import philox_ref as ph
import tree_ref as tref
from multidraft_ref import BONUS, MASS_TOL, RESIDUAL

SITE_GUMBEL = 5              # csrc/sd_device.h: kSiteGumbel
CHUNK = 2048
# |key_device - key_host| measured on the MI355X over tests/test_gpu_sample_distinct.py's grid, and 4x it
KEY_ERR_MEASURED = 1.5e-6
KEY_TOL = 4 * KEY_ERR_MEASURED


def gumbel_keys(w, seed, off, row):
    """fp64 keys ln w + g of the weights w [V] on global row `row` (-inf where w has no key)."""
    words = np.stack(ph.block(seed, off, row, SITE_GUMBEL, np.arange((len(w) + 3) // 4, dtype=np.uint64)), axis=1).reshape(-1)[:len(w)]
    u = ((words >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    w = np.asarray(w, dtype=np.float64)
    ok = (w >= 2.0 ** -126) & np.isfinite(w)      # the device gives a subnormal weight no key
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, np.log(np.where(ok, w, 1.0)) - np.log(-np.log(u)), -np.inf)


def gumbel_topk(w, k, seed, off, row):
    """(tokens [k] with -1 past the support, keys [k], close): the k largest keys in descending order, lowest index
    first among equals; close = ranks whose gap to the next key (up to rank k + 1) is below 2 KEY_TOL."""
    keys = gumbel_keys(w, seed, off, row)
    order = np.lexsort((np.arange(len(keys)), -keys))[:k + 1]
    order = [int(i) for i in order if keys[i] > -np.inf]
    tok = (order[:k] + [-1] * k)[:k]
    ks = [float(keys[i]) for i in order[:k]] + [-math.inf] * (k - len(order[:k]))
    close = [j for j in range(min(k, len(order) - 1)) if keys[order[j]] - keys[order[j + 1]] < 2 * KEY_TOL]
    return np.array(tok), np.array(ks), close


def walk(P, Q, tok, parent, accept, exact=False):
    """sd_verify_tree_swor's rule; arguments and namespace as tree_ref.walk (frac = r[x] / q~[x]; a weightless
    child is rejected without a call of accept and recorded with frac NaN).  Zq: fp32 sums of 2048-element
    chunks added in fp64 and f rounded to fp32, as the device forms them; exact: both in fp64 (the enumeration)."""
    ch = tref.children_of(parent)
    out = SimpleNamespace(n=0, path=[], last_node=-1, slot=0, status=BONUS, rejects=0, mass=math.nan, weights=None,
                          final_mass=math.nan, tests=[], last_slack=0.0, masses=[], mass_at=None)
    s = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while ch[s]:
            q, r = np.asarray(Q[s], dtype=np.float64), np.asarray(P[s], dtype=np.float64).copy()
            zq = float(q.sum()) if exact else sum(float(np.float32(q[c:c + CHUNK].sum())) for c in range(0, len(q), CHUNK))
            E, qe, slack = [], 0.0, 0.0
            for j, c in enumerate(ch[s]):
                x = int(tok[c])
                weighted = 0 <= x < len(r) and x not in E and q[x] > 0
                f = zq / (zq - qe) if weighted else 0.0
                qt = (f if exact else float(np.float32(f))) * q
                qt[E] = 0.0
                frac = float(r[x] / qt[x]) if weighted else math.nan
                acc = weighted and bool(accept(c, j, frac, slack))
                out.tests.append((c, j, frac, acc))
                if acc:
                    break
                if j == 0:                             # the slot's first rejection
                    out.masses, out.mass_at = [], s
                out.weights = np.maximum(r - qt, 0.0)
                out.mass = out.final_mass = float(out.weights.sum())
                r = out.weights / out.mass
                out.masses.append(out.mass)
                slack += MASS_TOL / out.mass if out.mass > 0 else math.inf
                out.rejects, out.last_slack = out.rejects + 1, slack
                if weighted:
                    E, qe = E + [x], qe + float(q[x])
            else:                                      # every child rejected
                out.n, out.slot, out.status = len(out.path), s, RESIDUAL
                return out
            out.path.append(c)
            out.last_node, s = c, c + 1
    out.n, out.slot, out.weights = len(out.path), s, np.asarray(P[s], dtype=np.float64)
    out.final_mass = float(out.weights.sum())
    return out


def under_rule(fn, *args, **walk_kw):
    """tests/tree_ref.py's fn (philox_step: close with q~ in the ratio; enumerate_outcomes) over this rule's walk."""
    saved, tref.walk = tref.walk, functools.partial(walk, **walk_kw)
    try:
        return fn(*args)
    finally:
        tref.walk = saved


def draw_children(Q, parent, seed, off, row_of_slot):
    """tok [N]: every internal slot's children are the Gumbel top-k draws of its row Q[s] on global row row_of_slot(s)."""
    tok = np.full(len(parent), -1, dtype=np.int64)
    for s, cs in enumerate(tref.children_of(parent)):
        if cs:
            tok[cs] = gumbel_topk(Q[s], len(cs), seed, off, row_of_slot(s))[0]
    return tok


def enumerate_joint(p_of, q_of, V, parent, forced=()):
    """The exact joint [V, V] of the first two tokens a step emits followed by the target itself: every ordered
    without-replacement assignment of every slot's children under q_of(prefix) by its probability, the nodes of `forced`
    then set to -1 (last siblings: a truncated draw), every outcome of walk() (accept uniforms integrated out) by its."""
    ch, N, joint = tref.children_of(parent), len(parent), np.zeros((V, V))

    def prefix_of(s, tok):
        return prefix_of(parent[s - 1] + 1, tok) + (int(tok[s - 1]),) if s else ()

    def finish(tok, prob):
        t = np.array(tok)
        t[list(forced)] = -1
        P, Q = (np.array([f(prefix_of(s, tok)) for s in range(N + 1)]) for f in (p_of, q_of))
        for pr, o in under_rule(tref.enumerate_outcomes, P, Q, t, parent, exact=True):
            acc, w = [int(t[c]) for c in o.path], o.weights / o.weights.sum()
            if len(acc) >= 2:
                joint[acc[0], acc[1]] += prob * pr
            elif acc:
                joint[acc[0]] += prob * pr * w
            else:
                joint[:] += prob * pr * w[:, None] * np.array([p_of((a,)) for a in range(V)])

    def assign(s, tok, prob):
        while s <= N and not ch[s]:
            s += 1
        if s > N:
            return finish(tok, prob)
        q = q_of(prefix_of(s, tok))
        for xs in itertools.permutations(range(V), len(ch[s])):
            pr, rest, t = 1.0, 1.0, list(tok)
            for c, x in zip(ch[s], xs):
                pr, rest, t[c] = pr * q[x] / rest, rest - q[x], x
            assign(s + 1, t, prob * pr)

    assign(0, [0] * N, 1.0)
    return joint
