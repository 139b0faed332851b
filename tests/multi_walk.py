"""Case builders of the multi-draft verify tests (tests/test_gpu_multidraft.py,
tests/test_gpu_multidraft_edges.py and the CPU test that proves their coverage): rows, drafts CHOSEN
by the test so that the walks reach the branches of the rule (as tests/perf_walk.py does for the
single-chain verify), the host model's result of every sequence (tests/multidraft_ref.py over the
exact-arithmetic oracle and the numpy Philox), and the bounds the device's mass and draw are held to.

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import multidraft_ref as mref
import philox_ref as ph
import row_edges as rowe
from oracle import specdec_ref as ref

PROCS = {
    "multinomial": ref.Processor("multinomial", 1.0),
    "multinomial_T0.7": ref.Processor("multinomial", 0.7),
    "topk50": ref.Processor("topk", 1.0, top_k=50),
    "nucleus0.9": ref.Processor("nucleus", 1.0, top_p=0.9, stable_ties=True),
    "topk50_nucleus0.9": ref.Processor("topknucleus", 1.0, top_k=50, top_p=0.9, stable_ties=True),
    "greedy": ref.Processor("greedy", 1.0),
}
SHAPES = [(1, 4), (2, 1), (2, 4), (3, 5), (4, 4), (8, 8), (2, 32)]      # (K, γ)
VOCABS = [1000, 4096, 50257]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
BATCHES = [16, 1, 3]
SEED, OFFSET, ROW_BASE = 0x5EED1234ABCD, 7, 5
MARGIN = 0.02           # a steered test's ratio stays this far from its uniform

# the scenarios a sequence's drafts are steered through (b % len): directives per depth over the alive
# chains in test order — "A" accept, "R" reject, "S" the token of the chain that was accepted (a
# same-token chain not yet tried), None: the iid draft stays
SCENARIOS = ("iid", "rej0", "rejD", "sib", "full")


def grid():
    """The GPU walk cases: every (K, γ) with every vocabulary; dtype, batch and processor cycle so
    that each (K, γ) meets every dtype and batch size and each processor every dtype.  The hinted
    variant (the draws' statistics and keeps) repeats each case."""
    cases = []
    names = list(PROCS)
    for i, (K, g) in enumerate(SHAPES):
        for j, V in enumerate(VOCABS):
            n = i * len(VOCABS) + j
            dtype, name = DTYPES[(i + 2 * j) % 3], names[n % len(names)]
            if dtype == torch.float16 and ("topk" in name or "nucleus" in name):
                # the reference's mask value (-1e20) does not fit fp16: its top-k / nucleus raise there
                name = "multinomial_T0.7" if n % 2 else "greedy"
            cases.append((BATCHES[(i + j) % 3], K, g, V, dtype, name))
    cases.append((3, 4, 4, 128256, torch.bfloat16, "multinomial"))
    # keep processors (threshold search, hinted keeps) on 16-sequence cases that reach every branch
    cases += [(16, 8, 8, 1000, torch.bfloat16, "topk50_nucleus0.9"), (16, 4, 4, 4096, torch.float32, "topk50_nucleus0.9"),
              (16, 2, 4, 4096, torch.bfloat16, "topk50"), (16, 3, 5, 4096, torch.float32, "nucleus0.9")]
    return cases


def feasible(K, g):
    """Which branches a (K, γ) can reach at all."""
    return SimpleNamespace(sib_deep=K >= 2 and g >= 2, rej0=True, rej_deep=g >= 2, full_other=K >= 2,
                           blocks=K * g > 4)


def _directive(scn, d, j, K=2):
    if K == 1 and scn == "full":
        return "A"
    if scn == "rej0":
        return "R" if d == 0 else None
    if scn == "rejD":
        return ("A" if j == 0 else "S") if d == 0 else ("R" if d == 1 else None)
    if scn == "sib":
        if d == 1:
            return "R" if j == 0 else ("A" if j == 1 else "S")
        return "A" if j == 0 else "S"
    if scn == "full":
        if d == 0:
            return "R" if j == 0 else ("A" if j == 1 else "S")
        return "A" if j == 0 else "S"
    return None


def _steer(P, Q, tok, scn, uni):
    """Overwrite tok [K, γ] along the walk so that it follows the scenario where the rows and the
    uniforms allow it (a directive that cannot be met with MARGIN leaves the iid draft; so does one
    met after a residual whose mass is zero, as small vocabularies have: nothing is left to steer by)."""
    K, g = tok.shape
    A = list(range(K))
    for d in range(g):
        k0 = A[0]
        q, r = Q[k0, d].astype(np.float64), P[k0, d].astype(np.float64).copy()
        ok = q >= 1e-4
        hit = None
        for j, k in enumerate(A):
            want = _directive(scn, d, j, K)
            u = float(uni[d * K + k])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(ok, r / q, np.nan)
            if np.isnan(ratio).all():
                want = None
            if want == "A" and np.nanmax(ratio) > u + MARGIN:
                tok[k, d] = int(np.nanargmax(ratio))
            elif want == "R" and np.nanmin(ratio) < u - MARGIN:
                tok[k, d] = int(np.nanargmin(ratio))
            x = int(tok[k, d])
            with np.errstate(divide="ignore", invalid="ignore"):
                frac = r[x] / q[x]
            if not (u > frac):
                hit = x
                for k2 in A[j + 1:]:
                    if _directive(scn, d, A.index(k2), K) == "S":
                        tok[k2, d] = x
                break
            diff = np.maximum(r - q, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = diff / diff.sum()
        if hit is None:
            return
        A = [k for k in A if int(tok[k, d]) == hit]


@functools.lru_cache(maxsize=4)
def case(B, K, g, V, dtype, proc_name, seed=11):
    """Rows tl [B, K, γ+1, V], dl [B, K, γ, V] (dl = tl + N(0, 0.7²), target logits randn * 3), the
    oracle's rounded probabilities P, Q (fp32 tensors holding dtype values), drafts tok [B, K, γ]
    drawn iid from Q and then steered by sequence b's scenario SCENARIOS[b % 5]."""
    gen = torch.Generator().manual_seed(seed * 1000003 + K * 101 + g * 7 + V)
    tl = (torch.randn(B, K, g + 1, V, generator=gen) * 3).to(dtype)
    dl = (tl[:, :, :g].float() + 0.7 * torch.randn(B, K, g, V, generator=gen)).to(dtype)
    return _with_drafts(tl, dl, proc_name, gen)


def _with_drafts(tl, dl, proc_name, gen, **extra):
    """The case of rows tl, dl: the oracle's P, Q and the steered drafts (see case)."""
    (B, K, g, V), dtype = dl.shape, tl.dtype
    proc = PROCS[proc_name]
    P = ref.process(tl, proc, exact=True).float()
    Q = ref.process(dl, proc, exact=True).float()
    tok = torch.multinomial(Q.reshape(-1, V), 1, generator=gen).reshape(B, K, g)
    for b in range(B):
        uni = [ph.accept_uniform(SEED, OFFSET, ROW_BASE + b, i) for i in range(K * g)]
        t = tok[b].numpy().copy()
        _steer(P[b].numpy(), Q[b].numpy(), t, SCENARIOS[b % len(SCENARIOS)], uni)
        tok[b] = torch.from_numpy(t)
    return SimpleNamespace(B=B, K=K, gamma=g, V=V, dtype=dtype, proc=proc, proc_name=proc_name, tl=tl, dl=dl, P=P, Q=Q,
                           tok=tok, **extra)


# ---------------------------------------------------------------- chunk edges of the draw
CHUNK = 2048            # elements per mass workgroup: the draw picks a chunk, then an element in it
EDGE_VOCABS = [2047, 2048, 2049, 4097, 6145]
EDGE_PROCS = ["multinomial", "multinomial_T0.7", "greedy"]
# input seeds of the edge cases for which 11 does not meet what tests/test_multidraft_cpu.py asks of
# them (draws on both sides of the last chunk's edge by both exits, no close row, a draw interval
# wider than its slack): the lowest seed above 11 that does.  Key: edge_grid()'s tuple
EDGE_SEEDS = {
    (16, 4, 2, 4097, torch.bfloat16, "greedy", True): 13,
    (16, 8, 2, 4097, torch.bfloat16, "multinomial", True): 18,
}


def last_chunk_start(V):
    return CHUNK * ((V - 1) // CHUNK)


def edge_grid():
    """The GPU cases at the chunk edges: V one below, at and above one chunk, and one above two and
    three, with the short last chunk boosted (`tail`) or not; dtype and processor cycle so that
    each dtype meets each processor.  The last case has 8 chains: draws after >= 2 rejections."""
    cases = []
    for V in EDGE_VOCABS:
        for tail in ((False, True) if V > CHUNK else (False,)):
            n = len(cases)
            cases.append((16, 4, 2, V, DTYPES[(n + n // 3) % 3], EDGE_PROCS[n % 3], tail))
    cases.append((16, 8, 2, 4097, torch.bfloat16, "multinomial", True))
    return cases


@functools.lru_cache(maxsize=4)
def edge_case(B, K, g, V, dtype, proc_name, tail):
    """As case; with `tail` the logits from last_chunk_start(V) on (the V - 2048 ((V-1) // 2048)
    elements of the short last chunk) get +8 in every target row, the bonus row included, and +6 in
    every drafter row: a large share of both the residual mass and the bonus mass lies in that chunk."""
    seed = EDGE_SEEDS.get((B, K, g, V, dtype, proc_name, tail), 11)
    gen = torch.Generator().manual_seed(seed * 1000003 + K * 101 + g * 7 + V)
    base = torch.randn(B, K, g + 1, V, generator=gen) * 3
    draft = base[:, :, :g] + 0.7 * torch.randn(B, K, g, V, generator=gen)
    if tail:
        base[..., last_chunk_start(V):] += 8
        draft[..., last_chunk_start(V):] += 6
    tl = base.to(dtype)
    dl = (tl[:, :, :g].float() + (draft - base[:, :, :g])).to(dtype)
    return _with_drafts(tl, dl, proc_name, gen, tail=tail)


# ---------------------------------------------------------------- small vocabularies, row layouts
SMALL_VOCABS = [1, 2, 3, 5, 7, 8, 9, 63, 65]
SMALL_PROCS = ["multinomial", "multinomial_T0.7", "greedy", "topk50", "nucleus0.9"]


def small_grid():
    """(B, K, γ, V, dtype, processor, mask, layout, hinted) of tests/test_gpu_multidraft_edges.py:
    every V with every layout and every dtype; mask, processor and the hinted variant cycle.  The
    keep processors run on bf16 and fp32 only (the reference's mask value does not fit fp16)."""
    cases = []
    for i, V in enumerate(SMALL_VOCABS):
        for j, layout in enumerate(rowe.LAYOUTS):
            for t, dtype in enumerate(DTYPES):
                n = len(cases)
                name = SMALL_PROCS[(n + i) % len(SMALL_PROCS)]
                if dtype == torch.float16 and ("topk" in name or "nucleus" in name):
                    name = EDGE_PROCS[(i + j) % 3]
                cases.append((16, 4, 2, V, dtype, name, rowe.MASKS[(i + j + t) % 3], layout, n % 3 == 0))
    for n, (K, g) in enumerate([(1, 1), (8, 1)]):
        for j, layout in enumerate(rowe.LAYOUTS):
            cases.append((16, K, g, 3, DTYPES[(n + j) % 3], EDGE_PROCS[(n + j) % 3], rowe.MASKS[j], layout, j == 1))
    return cases


@functools.lru_cache(maxsize=4)
def small_case(B, K, g, V, dtype, proc_name, mask):
    """As case on tests/row_edges.py's rows: target rows logits(mask) (`-inf` entries), drafter rows
    the target's plus N(0, 0.7²) — the same entries at `-inf`, so that the two rows' keeps agree and
    q > 0 wherever a draft is drawn."""
    seed = rowe.seed_of("multi", B, K, g, V, rowe.dt_name(dtype), proc_name, mask)
    tl = rowe.logits((B, K, g + 1, V), dtype, seed, mask)
    gen = torch.Generator().manual_seed(seed + 1)
    dl = (tl[:, :, :g].float() + 0.7 * torch.randn(B, K, g, V, generator=gen)).to(dtype)
    return _with_drafts(tl, dl, proc_name, gen, mask=mask)


def host_results(c, stops=(), seed=SEED, off=OFFSET, row_base=ROW_BASE):
    """The host model's step of every sequence of case c."""
    return [mref.philox_step(c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy(), seed, off,
                             row_base + b, stops, greedy=not c.proc.stochastic) for b in range(c.B)]


def coverage(c, rows):
    """What the host walks of a case reached."""
    K = c.K
    cov = SimpleNamespace(sib_deep=0, rej0=0, rej_deep=0, full_other=0, full=0, blocks=0, close=0, kept_untried=0,
                          readmit=0)
    for r in rows:
        cov.close += r.close
        cov.readmit += r.readmit
        cov.kept_untried += r.kept_untried
        cov.rej0 += r.status != mref.BONUS and r.n == 0 and r.x is not None
        cov.rej_deep += r.status == mref.RESIDUAL and r.n >= 1
        cov.full += r.status == mref.BONUS
        cov.full_other += r.status == mref.BONUS and r.winner != 0
        for d, k, j, frac, acc in r.tests:
            cov.sib_deep += acc and j >= 1 and d >= 1
            cov.blocks += acc and (d * K + k) >= 4
    return cov


def flip_slack(logits_rows, dtype):
    """Σ over the rows' elements of how far a rounded probability can move when its softmax
    normaliser is off by 1e-6 (relative), as tests/perf_walk.py's flip_slack, summed over rows."""
    v = torch.softmax(logits_rows.double(), dim=-1)
    return float(((v * (1 + 1e-6)).to(dtype).double() - (v * (1 - 1e-6)).to(dtype).double()).sum())


def _slack_of(c, row):
    y = ref.processed_logits(row, c.proc, exact=True) / c.proc.temperature
    return flip_slack(y, c.dtype)


def mass_tolerance(c, b, r):
    """The bound on |device mass - host mass| of the last residual formed: 1e-5 (the project's mass
    tolerance) plus flip_slack summed over the row pair the residual was formed from — how far the
    rounded probabilities of the target and the drafter row can move when their softmax normalisers
    are off by 1e-6.  The same bound whatever the number of rejected siblings."""
    k0, d = r.mass_at
    return 1e-5 + _slack_of(c, c.tl[b, k0, d]) + _slack_of(c, c.dl[b, k0, d])


def draw_slack(c, b, r):
    """The bound on how far any partial sum of the device's draw weights lies from the host's: the
    draw weights are the very terms the mass sums, so a residual exit takes mass_tolerance (of the
    row pair at r.mass_at); a bonus exit 1e-5 plus flip_slack of the winner's bonus row."""
    if r.status == mref.BONUS:
        return 1e-5 + _slack_of(c, c.tl[b, r.winner, c.gamma])
    return mass_tolerance(c, b, r)


def draw_excess(r, x, slack):
    """How far the host's target u·Σ lies outside the running-total interval of the token x the
    device returned, as a fraction of the allowed 2·slack (0 inside; the check passes up to 1): one
    slack covers the device's total, the other its running sum."""
    lo, hi = mref.draw_interval(r.weights, x)
    t = r.u * r.total
    return max(lo - t, t - hi, 0.0) / (2 * slack)


def draw_margins(c, rows):
    """[(b, slack, w[x], edge)] of the rows of a stochastic case that draw by inverse CDF on the host:
    the row's draw_slack, the weight of the host's token and the distance of the host's target u·Σ
    from the nearer end of that token's interval.  The GPU check's widened interval
    [lo - 2 slack, hi + 2 slack] says something where 4 slack < w[x], and admits a neighbouring token
    only where edge <= 2 slack."""
    out = []
    for b, r in enumerate(rows):
        if c.proc.stochastic and r.x is not None:
            t = r.u * r.total
            out.append((b, draw_slack(c, b, r), float(r.weights[r.x]), min(t - r.lo, r.hi - t)))
    return out


def pair_distribution(p0, q0, p1, K):
    """(w0 [V], w1 [V]): the exact distribution of (t0, t1) over sequences that accepted a draft at
    depth 0 (n >= 1), K chains drawn iid from q0, context-free rows: w0 ⊗ w1 up to normalisation.

    The residuals r_j = max(r_{j-1} - q, 0) / m_j do not depend on which token was rejected, and a
    test at ordinal j fails with probability 1 - Σ min(q, r_{j-1}) = m_j, so all K chains are rejected
    with probability Π m_j and the step then emits r_K.  The step as a whole emits p0 (losslessness of
    the node), hence P(t0 = a, n >= 1) = p0(a) - (Π m_j) r_K(a).  Whatever the alive set, depth 1 is
    again a lossless node on its own rows: t1 ~ p1."""
    r = np.asarray(p0, dtype=np.float64).copy()
    q = np.asarray(q0, dtype=np.float64)
    allrej = 1.0
    for _ in range(K):
        diff = np.maximum(r - q, 0.0)
        m = diff.sum()
        allrej *= m
        r = diff / m
    w0 = np.maximum(np.asarray(p0, dtype=np.float64) - allrej * r, 0.0)
    return w0, np.asarray(p1, dtype=np.float64)


# ---------------------------------------------------------------- the loop on FakeLM banks
def bank_rows(lm, tokens, positions, proc):
    """The oracle's rounded probabilities of a FakeLM's logit rows at (token, position) pairs
    (tests/fakelm.py: row (31 token + pos_mult position) mod rows of the bank), fp64 [n, V]."""
    idx = [(int(t) * 31 + int(p) * lm.pos_mult) % lm.bank.shape[0] for t, p in zip(tokens, positions)]
    return ref.process(lm.bank[idx].cpu(), proc, exact=True).double().numpy()


def step_rows(target, drafter, prev_token, cur, tok, proc):
    """(P [K, γ+1, V], Q [K, γ, V]) of one loop step: chain k's row d sits at position cur-1+d, whose
    token is the last emitted one (d = 0) or the chain's draft d-1."""
    K, g = tok.shape
    P, Q = [], []
    for k in range(K):
        at = [int(prev_token)] + [int(t) for t in tok[k]]
        pos = [cur - 1 + d for d in range(g + 1)]
        P.append(bank_rows(target, at, pos, proc))
        Q.append(bank_rows(drafter, at[:g], pos[:g], proc))
    return np.stack(P), np.stack(Q)


def simulate_acceptance(target, drafter, K, g, steps, seed, proc=None):
    """Mean accepted drafts per step of the multi-draft loop on a FakeLM pair, by the host model with
    numpy noise (drafts iid from the exact q): the gain the device loop can be expected to show."""
    proc = proc or PROCS["multinomial"]
    rng = np.random.default_rng(seed)
    rows = target.bank.shape[0]
    Pb = ref.process(target.bank.cpu(), proc, exact=True).double().numpy()
    Qb = ref.process(drafter.bank.cpu(), proc, exact=True).double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % rows   # noqa: E731
    prev, cur, total = 3, 8, 0
    for _ in range(steps):
        tok = np.zeros((K, g), dtype=np.int64)
        P, Q = np.zeros((K, g + 1, Pb.shape[1])), np.zeros((K, g, Pb.shape[1]))
        for k in range(K):
            t = prev
            for d in range(g):
                i = row(t, cur - 1 + d)
                P[k, d], Q[k, d] = Pb[i], Qb[i]
                t = tok[k, d] = rng.choice(len(Qb[i]), p=Qb[i] / Qb[i].sum())
            P[k, g] = Pb[row(t, cur - 1 + g)]
        o = mref.walk(P, Q, tok, lambda d, k, j, frac, slack: not (rng.random() > frac))
        total += o.n
        prev = rng.choice(len(o.weights), p=o.weights / o.weights.sum())
        cur += o.n + 1
    return total / steps
