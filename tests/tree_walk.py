"""Case builders of the token-tree verify tests (tests/test_gpu_tree.py and the CPU test that proves
their coverage, tests/test_tree_cpu.py): trees, rows, drafts CHOSEN by the test so that the walks
reach the branches of the rule (as tests/multi_walk.py does for the multi-draft verify), the host
model's result of every sequence (tests/tree_ref.py over the exact-arithmetic oracle and the numpy
Philox) and the bounds the device's mass and draw are held to (multi_walk's).

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import multi_walk as mw
import philox_ref as ph
import row_edges as rowe
import tree_ref as tref
from oracle import specdec_ref as ref

PROCS = mw.PROCS
SEED, OFFSET, ROW_BASE = mw.SEED, mw.OFFSET, mw.ROW_BASE
MARGIN = mw.MARGIN
CHUNK = mw.CHUNK
DTYPES = mw.DTYPES
VOCABS = [1, 2, 3, 64, 2047, 2048, 2049, 4097, 50257]


def chains(K, g):
    return [i - K if i >= K else -1 for i in range(K * g)]


def from_branching(widths):
    parent, level = [], [-1]
    for w in widths:
        nxt = []
        for p in level:
            for _ in range(w):
                nxt.append(len(parent))
                parent.append(p)
        level = nxt
    return parent


def irregular():
    """64 nodes: child counts cycle through an uneven list breadth-first (one slot with 8 children,
    leaves at depths 2 to 4)."""
    counts = [5, 8, 3, 0, 2, 1, 2, 0, 1, 3, 0, 1, 2, 0, 0, 1, 2, 1, 0, 3, 1, 0, 2, 1]
    parent, queue, i = [], [-1], 0
    while len(parent) < 64:
        p = queue.pop(0)
        want = counts[i % len(counts)] if queue or counts[i % len(counts)] else 1
        i += 1
        for _ in range(min(want, 64 - len(parent))):
            queue.append(len(parent))
            parent.append(p)
    return parent


TREES = {
    "one": [-1],
    "chain32": chains(1, 32),
    "fan8": from_branching([8]),
    "b4211": from_branching([4, 2, 1, 1]),
    "irregular64": irregular(),
}
# the scenarios a sequence's drafts are steered through (b % len): what the walk should do at each
# slot it reaches — "iid" leaves the drafts; "rej0" rejects every child of the root; "rejD" accepts the
# first child of the root and rejects every child below it; "last" rejects all but the last child of
# every slot (sibling rejects all the way to a leaf); "first" accepts the first child everywhere;
# "second" accepts the root's second child, then first children (another leaf, often another depth)
SCENARIOS = ("iid", "rej0", "rejD", "last", "first", "second")


def _directive(scn, depth, j, n_children):
    if scn == "rej0":
        return "R" if depth == 0 else None
    if scn == "rejD":
        return "A" if depth == 0 else ("R" if depth == 1 else None)
    if scn == "last":
        return "A" if j == n_children - 1 else "R"
    if scn == "first":
        return "A"
    if scn == "second":
        return ("R" if j == 0 and n_children > 1 else "A") if depth == 0 else "A"
    return None


def _steer(P, Q, tok, parent, scn, uni):
    """Overwrite tok [N] along the walk so that it follows the scenario where the rows and the
    uniforms allow it (a directive that cannot be met with MARGIN leaves the iid draft; so does one met
    after a residual whose mass is zero, as small vocabularies have: nothing is left to steer by)."""
    ch = tref.children_of(parent)
    s, depth = 0, 0
    while ch[s]:
        q, r = Q[s].astype(np.float64), P[s].astype(np.float64).copy()
        ok = q >= 1e-4
        hit = None
        for j, c in enumerate(ch[s]):
            want = _directive(scn, depth, j, len(ch[s]))
            u = float(uni[c])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(ok, r / q, np.nan)
            if np.isnan(ratio).all():
                want = None
            if want == "A" and np.nanmax(ratio) > u + MARGIN:
                tok[c] = int(np.nanargmax(ratio))
            elif want == "R" and np.nanmin(ratio) < u - MARGIN:
                tok[c] = int(np.nanargmin(ratio))
            x = int(tok[c])
            with np.errstate(divide="ignore", invalid="ignore"):
                frac = r[x] / q[x]
            if not (u > frac):
                hit = c
                break
            diff = np.maximum(r - q, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = diff / diff.sum()
        if hit is None:
            return
        s, depth = hit + 1, depth + 1


# input seeds of the grid cases for which 11 does not meet what tests/test_tree_cpu.py asks of them (every
# branch the tree allows, at most one close row): the lowest seed above 11 that does.  Key: case()'s arguments
GRID_SEEDS = {
    (1, "fan8", 2047, torch.float16, "multinomial", False, "none"): 13,
    (1, "b4211", 64, torch.bfloat16, "nucleus0.9", False, "none"): 13,
    (1, "irregular64", 50257, torch.float32, "multinomial", False, "none"): 12,
}
SEQS_B1 = 6             # a B = 1 case verifies this many sequences, one call each: one per scenario


def grid():
    """The GPU walk cases (B, tree, V, dtype, processor, tail): every tree with every vocabulary;
    dtype, processor and batch cycle so that each tree meets every dtype, both batch sizes and every
    processor.  V above one chunk gets the boosted last chunk of multi_walk.edge_case (but the
    largest).  B = 33: one call of 33 sequences; B = 1: SEQS_B1 calls of one sequence each (global
    rows ROW_BASE + b), so that a B = 1 case reaches the branches too.  B = 33 only where the host
    oracle's rows stay small (33 (N+1) V <= 6 Mi elements)."""
    cases = []
    names = list(PROCS)
    for i, (tname, parent) in enumerate(TREES.items()):
        for j, V in enumerate(VOCABS):
            n = i * len(VOCABS) + j
            dtype, name = DTYPES[(i + 2 * j) % 3], names[(n + i) % len(names)]
            if dtype == torch.float16 and ("topk" in name or "nucleus" in name):
                # the reference's mask value (-1e20) does not fit fp16: its top-k / nucleus raise there
                name = "multinomial_T0.7" if n % 2 else "greedy"
            B = 1 if (i + j) % 3 == 0 or 33 * (len(parent) + 1) * V > 6 << 20 else 33
            cases.append((B, tname, V, dtype, name, CHUNK < V < 50000))
    return cases


def n_seqs(B):
    return SEQS_B1 if B == 1 else B


@functools.lru_cache(maxsize=4)
def case(B, tname, V, dtype, proc_name, tail=False, mask="none"):
    """Rows tl [B, N+1, V] (target logits randn * 3 by slot), dl [B, N+1, V] (tl + N(0, 0.7²); read at
    internal slots only), the oracle's rounded probabilities P, Q (fp32 tensors holding dtype
    values), drafts tok [B, N] drawn iid from Q of the parent slot and then steered by sequence b's
    scenario SCENARIOS[b % 6]; B = 1 builds SEQS_B1 sequences (see grid).  With `tail` the logits from
    the last chunk's start on get +8 in the target rows and +6 in the drafter rows; `mask` puts `-inf` entries (tests/row_edges.py) into the
    target rows, and the drafter rows have them at the same places.  tname: a name of TREES, or a parent
    list given as a tuple."""
    parent = TREES[tname] if isinstance(tname, str) else list(tname)
    seed = GRID_SEEDS.get((B, tname, V, dtype, proc_name, tail, mask), 11)
    N, B = len(parent), n_seqs(B)
    gen = torch.Generator().manual_seed(seed * 1000003 + N * 101 + V)
    if mask != "none":
        base = rowe.logits((B, N + 1, V), torch.float32, rowe.seed_of("tree", B, tname, V, mask), mask)
    else:
        base = torch.randn(B, N + 1, V, generator=gen) * 3
    noise = 0.7 * torch.randn(B, N + 1, V, generator=gen)
    if tail:
        base[..., mw.last_chunk_start(V):] += 8
        noise[..., mw.last_chunk_start(V):] -= 2
    tl = base.to(dtype)
    dl = (tl.float() + noise).to(dtype)
    return with_drafts(tl, dl, parent, proc_name, gen, tname=tname, tail=tail, mask=mask)


def with_drafts(tl, dl, parent, proc_name, gen, **extra):
    (B, S, V), dtype = tl.shape, tl.dtype
    N = S - 1
    proc = PROCS[proc_name]
    P = ref.process(tl, proc, exact=True).float()
    Q = ref.process(dl, proc, exact=True).float()
    pslot = torch.tensor([p + 1 for p in parent])
    tok = torch.multinomial(Q[:, pslot].reshape(-1, V), 1, generator=gen).reshape(B, N)
    for b in range(B):
        uni = [ph.accept_uniform(SEED, OFFSET, ROW_BASE + b, i) for i in range(N)]
        t = tok[b].numpy().copy()
        _steer(P[b].numpy(), Q[b].numpy(), t, parent, SCENARIOS[b % len(SCENARIOS)], uni)
        tok[b] = torch.from_numpy(t)
    return SimpleNamespace(B=B, N=N, V=V, dtype=dtype, proc=proc, proc_name=proc_name, parent=parent, tl=tl, dl=dl, P=P, Q=Q,
                           tok=tok, **extra)


def host_results(c, stops=(), seed=SEED, off=OFFSET, row_base=ROW_BASE):
    """The host model's step of every sequence of case c."""
    return [tref.philox_step(c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy(), c.parent, seed, off,
                             row_base + b, stops, greedy=not c.proc.stochastic) for b in range(c.B)]


def node_depths(parent):
    d = []
    for p in parent:
        d.append(1 if p < 0 else d[p] + 1)
    return d


def coverage(c, rows):
    """What the host walks of a case reached."""
    cov = SimpleNamespace(resid_root=0, resid_deep=0, bonus_depths=set(), two_rejects=0, late_chunk=0, close=0)
    for r in rows:
        cov.close += r.close
        drawn = r.x is not None
        cov.resid_root += r.status == tref.RESIDUAL and r.n == 0 and drawn
        cov.resid_deep += r.status == tref.RESIDUAL and r.n >= 1
        if r.status == tref.BONUS:
            cov.bonus_depths.add(r.n)
        per_slot = {}
        for node, j, frac, acc in r.tests:
            if not acc:
                per_slot[c.parent[node]] = per_slot.get(c.parent[node], 0) + 1
        cov.two_rejects += any(v >= 2 for v in per_slot.values())
        cov.late_chunk += drawn and r.x >= CHUNK
    return cov


def feasible(parent, V):
    """Which branches a tree can reach at all."""
    ch = tref.children_of(parent)
    depths = node_depths(parent)
    leaf_depths = {depths[i] for i in range(len(parent)) if not ch[i + 1]}
    return SimpleNamespace(resid_deep=any(ch[i + 1] for i in range(len(parent))), bonus_depths=len(leaf_depths),
                           two_rejects=max(len(x) for x in ch) >= 2, late_chunk=V > CHUNK)


def mass_tolerance(c, b, r):
    """multi_walk.mass_tolerance's bound for the slot the last residual was formed at: 1e-5 plus
    flip_slack of its target and its drafter row."""
    s = r.mass_at
    return 1e-5 + mw._slack_of(c, c.tl[b, s]) + mw._slack_of(c, c.dl[b, s])


def draw_slack(c, b, r):
    """multi_walk.draw_slack's bound: a residual exit takes mass_tolerance, a bonus exit 1e-5 plus
    flip_slack of the leaf's target row."""
    if r.status == tref.BONUS:
        return 1e-5 + mw._slack_of(c, c.tl[b, r.slot])
    return mass_tolerance(c, b, r)


def simulate_acceptance(target, drafter, parent, steps, seed, proc=None):
    """Mean accepted drafts per target forward of the tree loop on a FakeLM pair, by the host model
    with numpy noise (children iid from the exact q of their parent slot), as
    multi_walk.simulate_acceptance for chains."""
    proc = proc or PROCS["multinomial"]
    rng = np.random.default_rng(seed)
    nrows = target.bank.shape[0]
    Pb = ref.process(target.bank.cpu(), proc, exact=True).double().numpy()
    Qb = ref.process(drafter.bank.cpu(), proc, exact=True).double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % nrows   # noqa: E731
    N, depths = len(parent), node_depths(parent)
    prev, cur, total = 3, 8, 0
    for _ in range(steps):
        tok = np.zeros(N, dtype=np.int64)
        idx = [row(prev, cur - 1)] + [0] * N
        for i in range(N):
            q = Qb[idx[parent[i] + 1]]
            tok[i] = rng.choice(len(q), p=q / q.sum())
            idx[i + 1] = row(tok[i], cur - 1 + depths[i])
        o = tref.walk(Pb[idx], Qb[idx], tok, parent, lambda c, j, frac, slack: not (rng.random() > frac))
        total += o.n
        prev = rng.choice(len(o.weights), p=o.weights / o.weights.sum())
        cur += o.n + 1
    return total / steps
