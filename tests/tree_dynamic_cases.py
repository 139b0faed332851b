"""Case builders of the dynamic draft tree tests (tests/test_gpu_tree_grow.py): the grid of shapes, the
logit rows of every level, and the host model's result (tests/tree_dynamic_ref.py) of every sequence.
The input seed of a case is chosen ON THE HOST so that no decision that depends on score arithmetic
— a frontier boundary or the final-N boundary — sits within tree_dynamic_ref.CLOSE of a tie; exact
ties (equal logits under one parent) are decided by pool index on both sides and are not close.

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

import tree_dynamic_ref as yref

VOCABS = (5, 2048, 2049, 4097)
BATCHES = (1, 3)
SHAPES = ((1, 1), (2, 3), (8, 8))          # (W, c); c is cut to V where the vocabulary is smaller (c = V)
LEVELS = (1, 2, 5)
NODES = (1, 7, 64)                         # cut to the pool where it is smaller
DTYPES = (torch.bfloat16, torch.float32)
LAYOUTS = ("packed", "padded", "shifted")
SEED_LIMIT = 64


def grid():
    """(V, B, W, c, L, N, dtype, layout): every vocabulary with every (W, c) and every depth; batch, N,
    dtype and layout cycle so that every value of each meets every vocabulary."""
    cases = []
    for i, V in enumerate(VOCABS):
        for j, (W, c) in enumerate(SHAPES):
            for k, L in enumerate(LEVELS):
                n = (i * len(SHAPES) + j) * len(LEVELS) + k
                c_ = min(c, V)
                pool = yref.shape(L, W, c_)[1][-1]
                cases.append((V, BATCHES[(i + j + k) % 2], W, c_, L, min(NODES[(i + j + 2 * k) % 3], pool),
                              DTYPES[(i + k) % 2], LAYOUTS[n % 3]))
    return cases


def rows_of(seed, B, V, W, c, L, dtype, mask=False):
    """Per level the frontier's rows [B, F_{l-1}, V]: N(0, 3^2) logits; mask: half of every row at -inf."""
    g = torch.Generator().manual_seed(seed * 7919 + V * 31 + L)
    F, _ = yref.shape(L, W, c)
    out = []
    for l in range(L):
        x = torch.randn(B, F[l], V, generator=g) * 3
        if mask:
            for r in x.view(-1, V):
                r[torch.randperm(V, generator=g)[:V // 2]] = -math.inf
        out.append(x.to(dtype))
    return out


def host(rows, W, c, N):
    """The host model of every sequence."""
    B = rows[0].shape[0]
    return [yref.model([r[b] for r in rows], W, c, N) for b in range(B)]


@functools.lru_cache(maxsize=None)
def case(V, B, W, c, L, N, dtype, mask=False):
    """The case at its lowest input seed at which no sequence is close."""
    for seed in range(SEED_LIMIT):
        rows = rows_of(seed, B, V, W, c, L, dtype, mask)
        models = host(rows, W, c, N)
        if not any(m.close for m in models):
            return SimpleNamespace(V=V, B=B, W=W, c=c, L=L, N=N, dtype=dtype, seed=seed, rows=rows, models=models)
    raise LookupError(f"no seed below {SEED_LIMIT} without a close boundary: {(V, B, W, c, L, N, dtype, mask)}")
