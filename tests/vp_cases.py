"""Case builders of the vocabulary-parallel verify tests (tests/test_gpu_vocab_parallel.py and the
CPU test that proves their coverage, tests/test_vocab_parallel_cpu.py): whole rows, the partition
into slices, drafts CHOSEN by the test so that the walks reach every exit and the drafted ids sit on
slice edges, and the host model's result of every sequence (tests/vocab_parallel_ref.py over the
exact-arithmetic oracle and the numpy Philox).

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import multi_walk as mw
import philox_ref as ph
import vocab_parallel_ref as vref
from oracle import specdec_ref as ref

PROCS = {name: mw.PROCS[name] for name in ("multinomial", "multinomial_T0.7", "greedy")}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
BATCHES = [16, 1, 5]
GAMMAS = [0, 1, 4, 32]
SEED, OFFSET, ROW_BASE = 0x5EED7654CAFE, 11, 3
# the smallest layouts at which the kernels can still go wrong: one element per shard; one-element
# shards around a ragged one; a 2048-element chunk exactly, then one element; a slice of more than
# one chunk with a ragged end, a one-chunk slice that starts 2-byte aligned, a one-element tail;
# several chunks per slice, uneven by one; the serving shape
LAYOUTS = [(8, (1,) * 8), (37, (1, 35, 1)), (2049, (2048, 1)), (4100, (2051, 2048, 1)),
           (50257, tuple(vref.even_sizes(3, 50257)))]
BIG = (128256, tuple(vref.even_sizes(8, 128256)))
SCENARIOS = mw.SCENARIOS            # per sequence: iid, reject at 0, reject at depth 1, (sib = iid at K = 1), full accept


def grid():
    """(B, γ', V, sizes, dtype, processor, neg_inf, with_stop) of every GPU case: each layout with each
    γ'; batch, dtype and processor cycle so that each layout meets every batch size, dtype and
    processor; every third case has -inf entries (a whole slice of them in some sequences), every
    fourth a stop list that an accepted draft hits.  V = 128256 over 8 even shards once per dtype."""
    cases, names = [], list(PROCS)
    for i, (V, sizes) in enumerate(LAYOUTS):
        for j, g in enumerate(GAMMAS):
            n = i * len(GAMMAS) + j
            B = BATCHES[(i + j) % 3]
            if V > 5000 and g == 32:
                B = 1                                   # 65 rows of 50257: the host oracle's time
            cases.append((B, g, V, sizes, DTYPES[(i + 2 * j) % 3], names[(n + i) % 3], n % 3 == 1, g > 0 and n % 4 == 2))
    for k, dt in enumerate(DTYPES):
        cases.append((1 if k else 5, 4, BIG[0], BIG[1], dt, names[k], k == 2, k == 1))
    return cases


def case_id(c):
    B, g, V, sizes, dt, name, ninf, stop = c
    return f"B{B}-g{g}-V{V}-S{len(sizes)}-{str(dt).split('.')[-1]}-{name}" + ("-ninf" if ninf else "") + \
        ("-stop" if stop else "")


def _edge_tokens(tok, b, sizes, V):
    """Put drafted ids of sequence b on slice edges: the first element of a slice at depth 0 and the
    last element of a slice at the last depth (sequences 1 and 2 of a case; one-element slices are
    both at once)."""
    g = tok.shape[1]
    if g == 0:
        return
    bs = vref.bounds(sizes)
    o, n = bs[(b + 1) % len(bs)]
    if b % 5 == 1:
        tok[b, 0] = o                                   # first element of a slice
    elif b % 5 == 2:
        tok[b, g - 1] = o + n - 1                       # last element of a slice


@functools.lru_cache(maxsize=4)
def case(B, g, V, sizes, dtype, proc_name, neg_inf=False, with_stop=False, seed=23):
    """Whole rows tl [B, γ+1, V], dl [B, γ, V] (dl = tl + N(0, 0.7²), target logits randn * 3), the
    oracle's rounded probabilities P, Q, drafts tok [B, γ] drawn iid from Q, steered by sequence b's
    scenario, then put on slice edges; stops: a stop list (an accepted draft of a full-accept
    sequence) or ().  neg_inf: -inf logits sprinkled over every row, and in every other sequence one
    whole slice of -inf (target and drafter rows alike: its mass is 0)."""
    proc = PROCS[proc_name]
    gen = torch.Generator().manual_seed(seed * 1000003 + g * 7 + V + 13 * B)
    tl = torch.randn(B, g + 1, V, generator=gen) * 3
    noise = 0.7 * torch.randn(B, g, V, generator=gen)
    bs = vref.bounds(sizes)
    dead = [None] * B
    if neg_inf:
        tl[torch.rand(B, g + 1, V, generator=gen) < 0.1] = -float("inf")
        for b in range(0, B, 2):
            s = (b // 2 + 1) % len(bs)
            if len(bs) > 1:
                o, n = bs[s]
                tl[b, :, o:o + n] = -float("inf")
                dead[b] = s
        # keep every row alive: element 0 of the first live slice is finite
        for b in range(B):
            o = bs[0][0] if dead[b] != 0 else bs[1][0]
            tl[b, :, o] = 1.0
    tl = tl.to(dtype)
    dl = (tl[:, :g].float() + noise).to(dtype)
    P = ref.process(tl, proc, exact=True).float()
    Q = ref.process(dl, proc, exact=True).float() if g else torch.zeros(B, 0, V)
    tok = torch.multinomial(Q.reshape(-1, V), 1, generator=gen).reshape(B, g) if g else torch.zeros(B, 0, dtype=torch.long)
    idx = (V + g + B) % len(SCENARIOS)
    for b in range(B):
        if g == 0:
            break
        uni = [ph.accept_uniform(SEED, OFFSET, ROW_BASE + b, i) for i in range(g)]
        t = tok[b].numpy().copy()[None]
        scn = SCENARIOS[(b + idx) % len(SCENARIOS)]
        mw._steer(P[b].numpy()[None], Q[b].numpy()[None], t, scn, uni)
        tok[b] = torch.from_numpy(t[0])
        if scn == "iid":
            _edge_tokens(tok, b, sizes, V)
    stops = ()
    if with_stop and g:
        full = [b for b in range(B) if SCENARIOS[(b + idx) % len(SCENARIOS)] == "full"]
        b = full[0] if full else 0
        stops = (V + 5, int(tok[b, 0]))                 # a stop that never occurs is listed first
    return SimpleNamespace(B=B, gamma=g, V=V, sizes=tuple(sizes), dtype=dtype, proc=proc, proc_name=proc_name, tl=tl, dl=dl,
                           P=P, Q=Q, tok=tok, stops=stops, dead=dead, neg_inf=neg_inf)


def host_results(c, seed=SEED, off=OFFSET, row_base=ROW_BASE, sizes=None):
    """The host model's step of every sequence of case c (under another partition if sizes is given)."""
    return [vref.step(c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy(), seed, off, row_base + b,
                      sizes or c.sizes, c.stops, greedy=not c.proc.stochastic) for b in range(c.B)]


def coverage(c, rows):
    """What the host steps of a case reached."""
    bs = vref.bounds(c.sizes)
    S = len(bs)
    cov = SimpleNamespace(rej0=0, rej_deep=0, bonus=0, stop=0, close=0, tok_first=0, tok_last=0, one_elem_owner=0,
                          owner_first=0, owner_last=0, owner_mid=0, dead_slices=0)
    for b, r in enumerate(rows):
        cov.close += bool(r.close)
        cov.rej0 += r.status == "residual" and r.n == 0 and c.gamma > 0
        cov.rej_deep += r.status == "residual" and 0 < r.n < c.gamma
        cov.bonus += r.status == "bonus"
        cov.stop += r.status == "stop"
        for t in c.tok[b].tolist():
            for o, n in bs:
                if o <= t < o + n:
                    cov.tok_first += t == o
                    cov.tok_last += t == o + n - 1
                    cov.one_elem_owner += n == 1
        if r.owner is not None:
            cov.owner_first += r.owner == 0
            cov.owner_last += r.owner == S - 1
            cov.owner_mid += 0 < r.owner < S - 1
        if r.masses is not None:
            cov.dead_slices += int((np.asarray(r.masses) == 0).sum())
    return cov
