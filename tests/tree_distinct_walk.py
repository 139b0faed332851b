"""Case builders of the distinct-children tree verify tests (tests/test_gpu_tree_distinct.py): trees,
target rows, children taken as the top-c tokens of a correlated drafter row, target rows then STEERED
per sequence so that the walks reach the branches of the rule, the host model's result of every
sequence (tests/tree_distinct_ref.py over the exact-arithmetic oracle and the numpy Philox) and the
bounds the device's mass and draw are held to (multi_walk's).

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import multi_walk as mw
import tree_distinct_ref as dref
import tree_walk as tw
from oracle import specdec_ref as ref
from tree_ref import children_of

PROCS = mw.PROCS
SEED, OFFSET, ROW_BASE = mw.SEED, mw.OFFSET, mw.ROW_BASE
CHUNK = mw.CHUNK
DTYPES = mw.DTYPES
B = 8
TREES = {
    "one": [-1],
    "five": [-1, -1, 0, 0, 1],
    "fan8": tw.from_branching([8]),
    "two-two": tw.from_branching([2, 2]),
    "chain32": tw.chains(1, 32),
    "irregular64": tw.irregular(),
}
VOCABS = [1, 64, 1000, 2049, 4101]
PROC_NAMES = ["multinomial", "greedy", "topk50", "nucleus0.9"]
# what a sequence's target rows are steered to (b % len): "top" leaves them; "last" lifts the last
# child's token of every slot by 8 (earlier siblings are rejected, paths run deep); "first" lifts the
# first child's; "rej" lowers every child's token by 12 (residual exits, tiny excluded weights)
SCENARIOS = ("top", "last", "rej", "first")


def grid():
    """(tree, V, dtype, processor): every tree with every vocabulary; dtype and processor cycle.  The
    keep processors run on bf16 and fp32 only (the reference's mask value does not fit fp16)."""
    cases = []
    for i, tname in enumerate(TREES):
        for j, V in enumerate(VOCABS):
            n = i * len(VOCABS) + j
            dtype, name = DTYPES[(i + 2 * j) % 3], PROC_NAMES[(i + j) % len(PROC_NAMES)]
            if dtype == torch.float16 and ("topk" in name or "nucleus" in name):
                name = "multinomial" if n % 2 else "greedy"
            cases.append((tname, V, dtype, name))
    return cases


def top_children(dl, parent):
    """tok [B, N]: child j of a slot gets the (j+1)-th best token of the slot's row of dl [B, N+1, V]
    (value descending, lowest index first).  Where the slot has more children than the vocabulary has
    tokens, the rest get ids outside [0, V): V and -1 in turn."""
    Bn, _, V = dl.shape
    ch = children_of(parent)
    tok = torch.zeros(Bn, len(parent), dtype=torch.long)
    for s, cs in enumerate(ch):
        if not cs:
            continue
        for b in range(Bn):
            best = dref.topk_tokens(dl[b, s].double().numpy(), min(len(cs), V))
            for j, c in enumerate(cs):
                tok[b, c] = best[j] if j < len(best) else (V if (j - len(best)) % 2 == 0 else -1)
    return tok


def finish(tl, tok, parent, proc_name, **extra):
    """The case of rows tl [B, N+1, V] and children tok: the oracle's rounded probabilities P and, for
    greedy, the processed logits Y."""
    proc = PROCS[proc_name]
    P = ref.process(tl, proc, exact=True).double()
    Y = None if proc.stochastic else (ref.processed_logits(tl, proc, exact=True) / proc.temperature).double()
    return SimpleNamespace(B=tl.shape[0], N=len(parent), V=tl.shape[-1], dtype=tl.dtype, proc=proc, proc_name=proc_name,
                           parent=parent, tl=tl, tok=tok, P=P, Y=Y, **extra)


@functools.lru_cache(maxsize=4)
def case(tname, V, dtype, proc_name, seed=11):
    """tname: a name of TREES, or a parent list given as a tuple."""
    parent = TREES[tname] if isinstance(tname, str) else list(tname)
    N = len(parent)
    gen = torch.Generator().manual_seed(seed * 1000003 + N * 101 + V)
    base = torch.randn(B, N + 1, V, generator=gen) * 3
    if V > CHUNK:                                      # odd sequences: much of the mass in the short last chunk
        base[1::2, :, mw.last_chunk_start(V):] += 8
    dl = (base.to(dtype).float() + 0.7 * torch.randn(B, N + 1, V, generator=gen)).to(dtype)
    tok = top_children(dl, parent)
    ch = children_of(parent)
    for b in range(B):
        scn = SCENARIOS[b % len(SCENARIOS)]
        for s, cs in enumerate(ch):
            ids = [int(tok[b, c]) for c in cs if 0 <= int(tok[b, c]) < V]
            if not ids or scn == "top":
                continue
            if scn == "rej":
                base[b, s, ids] -= 12
            else:
                base[b, s, ids[-1] if scn == "last" else ids[0]] += 8
    return finish(base.to(dtype), tok, parent, proc_name, tname=tname)


def host_results(c, stops=(), seed=SEED, off=OFFSET, row_base=ROW_BASE):
    """The host model's step of every sequence of case c."""
    return [dref.philox_step(c.P[b].numpy(), c.tok[b].numpy(), c.parent, seed, off, row_base + b, stops,
                             Y=None if c.Y is None else c.Y[b].numpy()) for b in range(c.B)]


def quiet_offset(c, stops=(), start=OFFSET, limit=16):
    """(offset, rows): the lowest Philox offset from `start` on at which at most one row of the case sits
    close to an accept threshold — chosen on the host, before anything runs on the device."""
    for off in range(start, start + limit):
        rows = host_results(c, stops, off=off)
        if sum(r.close for r in rows) <= 1:
            return off, rows
    raise LookupError("no offset without close rows")


def mass_tolerance(c, b, slot):
    """multi_walk.mass_tolerance's bound with one row: 1e-5 plus flip_slack of the slot's target row
    (how far its rounded probabilities can move when the softmax normaliser is off by 1e-6).  Every
    quantity of this rule — Z, the excluded weights, rem — is a sum of those probabilities."""
    return 1e-5 + mw._slack_of(c, c.tl[b, slot])


def coverage(rows):
    cov = SimpleNamespace(resid_root=0, resid_deep=0, bonus=0, two_rejects=0, late_chunk=0, close=0, weightless=0)
    for r in rows:
        cov.close += r.close
        cov.resid_root += r.status == dref.RESIDUAL and r.n == 0
        cov.resid_deep += r.status == dref.RESIDUAL and r.n >= 1
        cov.bonus += r.status == dref.BONUS
        cov.two_rejects += len(r.excluded) >= 2
        cov.late_chunk += r.x is not None and r.x >= CHUNK
        cov.weightless += r.rejects > sum(not acc for _, _, _, acc in r.tests)
    return cov


def simulate_acceptance(target, drafter, parent, steps, seed, proc=None, greedy=False):
    """Mean accepted drafts per target forward of the tree loop with children="topk" on a FakeLM pair,
    by the host model with numpy noise: the children of a slot are the top-c tokens of the drafter's
    bank row, the walk tests/tree_distinct_ref.py's.  Compare tree_walk.simulate_acceptance (iid)."""
    proc = proc or PROCS["greedy" if greedy else "multinomial"]
    rng = np.random.default_rng(seed)
    nrows = target.bank.shape[0]
    tb = target.bank.cpu()
    Pb = ref.process(tb, proc, exact=True).double().numpy()
    Yb = tb.double().numpy()
    Db = drafter.bank.cpu().double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % nrows   # noqa: E731
    N, depths, ch = len(parent), tw.node_depths(parent), children_of(parent)
    prev, cur, total = 3, 8, 0
    for _ in range(steps):
        tok = np.zeros(N, dtype=np.int64)
        idx = [row(prev, cur - 1)] + [0] * N
        for s in range(N + 1):                         # parents come before their children
            if ch[s]:
                best = dref.topk_tokens(Db[idx[s]], len(ch[s]))
                for j, c in enumerate(ch[s]):
                    tok[c] = best[j]
                    idx[c + 1] = row(tok[c], cur - 1 + depths[c])
        o = dref.walk(Pb[idx], tok, parent, lambda c, j, ratio: not (rng.random() > ratio), Yb[idx] if greedy else None)
        total += o.n
        prev = int(np.argmax(Yb[idx[o.slot]])) if greedy else rng.choice(len(o.weights), p=o.weights / o.weights.sum())
        cur += o.n + 1
    return total / steps
