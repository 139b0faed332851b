"""Host model of the dynamic draft trees (sd_tree_grow, sd_tree_select): fp64 torch on the
CPU.  The growth rule level by level, the rerank, and how close every decision that depends on score
arithmetic sat to its boundary (the device adds fp32 log-probabilities; the tests choose cases on the
host in which no boundary is nearer than CLOSE).  The walk is tests/tree_distinct_ref.py's.

Everything here runs on the host.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import tree_distinct_ref as dref

CLOSE = 1e-3        # a frontier or final-N boundary whose two scores differ by at most this (and are not equal)
SCORE_TOL = 1e-4    # device fp32 scores against these fp64 ones


def shape(levels, width, branch):
    """(frontier sizes F_0..F_L, pool bases base_1..base_{L+1}): F_0 = 1, F_l = min(W, F_{l-1} c)."""
    F, base = [1], [0]
    for _ in range(levels):
        base.append(base[-1] + F[-1] * branch)
        F.append(min(width, F[-1] * branch))
    return F, base


def best_of(scores, k):
    """(the k best indices by (score descending, index ascending) in ASCENDING index, the gap between the
    last taken and the first left out: inf when nothing is left out, 0 for an exact tie)."""
    order = sorted(range(len(scores)), key=lambda i: (-scores[i] if scores[i] == scores[i] else math.inf, i))
    gap = math.inf
    if k < len(scores):
        a, b = scores[order[k - 1]], scores[order[k]]
        gap = 0.0 if a == b else a - b
    return sorted(order[:k]), gap


def grow_level(rows, pscore, ppool, base, width, branch):
    """One level.  rows [F, V] (any float dtype): the frontier's logit rows; pscore / ppool: the frontier
    nodes' scores and pool indices.  Returns the level's candidates (token, score, parent lists in pool
    order), the next frontier as indices INTO THIS LEVEL (ascending), and the boundary gap."""
    x = rows.double()
    lp = torch.log_softmax(x, -1).clamp(max=0.0)
    tok, score, parent = [], [], []
    for r in range(x.shape[0]):
        for t in dref.topk_tokens(x[r].numpy(), branch):
            tok.append(t)
            score.append(float(pscore[r]) + float(lp[r, t]))
            parent.append(int(ppool[r]))
    nxt, gap = best_of(score, min(width, len(score)))
    return SimpleNamespace(token=tok, score=score, parent=parent, frontier=nxt, gap=gap, base=base)


def grow(rows_of, levels, width, branch):
    """The whole pool.  rows_of(level, frontier) -> [F_{level-1}, V] logits, frontier a list of
    namespaces (pool, token, parent_rank, path: the tokens from the root's child down to the node; the
    root: an empty list with one implicit entry).  Returns pool (token, score, parent lists), frontiers
    (per level: token, pool, parent_rank lists) and gap (the smallest nonzero-or-zero boundary gap)."""
    pool = SimpleNamespace(token=[], score=[], parent=[], path=[])
    frontier = [SimpleNamespace(pool=-1, token=None, parent_rank=-1, path=())]
    out, gaps = [], []
    for level in range(1, levels + 1):
        rows = rows_of(level, frontier)
        base = len(pool.token)
        lv = grow_level(rows, [0.0 if f.pool < 0 else pool.score[f.pool] for f in frontier], [f.pool for f in frontier],
                        base, width, branch)
        for e, (t, s, p) in enumerate(zip(lv.token, lv.score, lv.parent)):
            pool.token.append(t); pool.score.append(s); pool.parent.append(p)
            pool.path.append(frontier[e // branch].path + (t,))
        frontier = [SimpleNamespace(pool=base + e, token=lv.token[e], parent_rank=e // branch, path=pool.path[base + e])
                    for e in lv.frontier]
        out.append(SimpleNamespace(token=[f.token for f in frontier], pool=[f.pool for f in frontier],
                                   parent_rank=[f.parent_rank for f in frontier]))
        gaps.append(lv.gap)
    return SimpleNamespace(pool=pool, frontiers=out, gaps=gaps)


def select(pool, num_nodes):
    """The rerank: tokens, parent (final indices), depth (1-based), pool_index, anc (python ints) of the
    num_nodes best pool entries in ascending pool index, and the boundary gap."""
    chosen, gap = best_of(pool.score, num_nodes)
    final = {p: i for i, p in enumerate(chosen)}
    parent = [final.get(pool.parent[p], -1) if pool.parent[p] >= 0 else -1 for p in chosen]
    closed = all(pool.parent[p] < 0 or pool.parent[p] in final for p in chosen)
    depth, anc = [], []
    for i, p in enumerate(parent):
        depth.append(1 if p < 0 else depth[p] + 1)
        anc.append((1 << i) | (0 if p < 0 else anc[p]))
    return SimpleNamespace(tokens=[pool.token[p] for p in chosen], parent=parent, depth=depth, pool_index=chosen, anc=anc,
                           gap=gap, closed=closed, path=[pool.path[p] for p in chosen] if getattr(pool, "path", None) else None)


def model(level_rows, width, branch, num_nodes):
    """grow + select of ONE sequence on given rows: level_rows[l] is [F_l, V], the rows of level l + 1's
    frontier whatever the tokens are (the kernels' tests).  close: a boundary gap in (0, CLOSE]."""
    g = grow(lambda level, frontier: level_rows[level - 1], len(level_rows), width, branch)
    s = select(g.pool, num_nodes)
    gaps = g.gaps + [s.gap]
    close = any(0 < x <= CLOSE or x != x for x in gaps)
    return SimpleNamespace(grow=g, sel=s, close=close, gaps=gaps)


def transitive_closure(parent):
    """anc by definition: bit k of entry i iff k == i or k is an ancestor of i."""
    out = []
    for i in range(len(parent)):
        a, k = 0, i
        while k >= 0:
            a |= 1 << k
            k = parent[k]
        out.append(a)
    return out


def brute_force(rows_of_ctx, V, levels, width, branch, num_nodes):
    """An independent enumeration of the EAGLE-2 pool for small V and L: every token path up to `levels`
    deep with its cumulative log-probability (dict of tuples, no pool indices), the expansion of the
    `width` best paths per level, and the `num_nodes` best candidates overall.  Returns (the set of
    selected paths, the list of frontier path sets per level, candidate path -> score).  Assumes no
    exact score ties (random rows)."""
    score = {}
    for n in range(1, levels + 1):
        for path in np.ndindex(*([V] * n)):
            ctx = path[:-1]
            x = np.asarray(rows_of_ctx(tuple(ctx)), dtype=np.float64)
            lp = x - x.max() - math.log(np.exp(x - x.max()).sum())
            score[tuple(path)] = (score[tuple(ctx)] if ctx else 0.0) + min(float(lp[path[-1]]), 0.0)
    frontier, cands, fronts = {()}, {}, []
    for _ in range(levels):
        level = {}
        for ctx in frontier:
            x = np.asarray(rows_of_ctx(ctx), dtype=np.float64)
            kids = sorted(range(V), key=lambda t: (-x[t], t))[:branch]
            for t in kids:
                level[ctx + (t,)] = score[ctx + (t,)]
        cands.update(level)
        frontier = set(sorted(level, key=lambda p: -level[p])[:width])
        fronts.append(frontier)
    chosen = set(sorted(cands, key=lambda p: -cands[p])[:num_nodes])
    return chosen, fronts, cands
