"""Case builders of the multi-draft verify tests (tests/test_gpu_multidraft.py and the CPU test that
proves their coverage): rows, drafts CHOSEN by the test so that the walks reach the branches of the
rule (as tests/perf_walk.py does for the single-chain verify), and the host model's result of every
sequence (tests/multidraft_ref.py over the exact-arithmetic oracle and the numpy Philox).

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import multidraft_ref as mref
import philox_ref as ph
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
    uniforms allow it (a directive that cannot be met with MARGIN leaves the iid draft)."""
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
            r = diff / diff.sum()
        if hit is None:
            return
        A = [k for k in A if int(tok[k, d]) == hit]


@functools.lru_cache(maxsize=4)
def case(B, K, g, V, dtype, proc_name, seed=11):
    """Rows tl [B, K, γ+1, V], dl [B, K, γ, V] (dl = tl + N(0, 0.7²), target logits randn * 3), the
    oracle's rounded probabilities P, Q (fp32 tensors holding dtype values), drafts tok [B, K, γ]
    drawn iid from Q and then steered by sequence b's scenario SCENARIOS[b % 5]."""
    proc = PROCS[proc_name]
    gen = torch.Generator().manual_seed(seed * 1000003 + K * 101 + g * 7 + V)
    tl = (torch.randn(B, K, g + 1, V, generator=gen) * 3).to(dtype)
    dl = (tl[:, :, :g].float() + 0.7 * torch.randn(B, K, g, V, generator=gen)).to(dtype)
    P = ref.process(tl, proc, exact=True).float()
    Q = ref.process(dl, proc, exact=True).float()
    tok = torch.multinomial(Q.reshape(-1, V), 1, generator=gen).reshape(B, K, g)
    for b in range(B):
        uni = [ph.accept_uniform(SEED, OFFSET, ROW_BASE + b, i) for i in range(K * g)]
        t = tok[b].numpy().copy()
        _steer(P[b].numpy(), Q[b].numpy(), t, SCENARIOS[b % len(SCENARIOS)], uni)
        tok[b] = torch.from_numpy(t)
    return SimpleNamespace(B=B, K=K, gamma=g, V=V, dtype=dtype, proc=proc, proc_name=proc_name, tl=tl, dl=dl, P=P, Q=Q,
                           tok=tok)


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
