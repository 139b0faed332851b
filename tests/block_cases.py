"""Case builders of the block verify tests (tests/test_gpu_block.py and the CPU test that proves their
coverage): rows, drafts CHOSEN by the builder so that the host model (tests/block_ref.py over the
exact-arithmetic oracle and the numpy Philox) reaches each scenario of the rule, the host model's result
of every sequence, and the bounds the device is held to — in the manner of tests/multi_walk.py.

Everything here runs on the host; cases are cached and shared: callers must not modify them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import block_ref as br
import multi_walk as mw
import multidraft_ref as mref
import philox_ref as ph
import row_edges as rowe
from oracle import specdec_ref as ref

PROCS = mw.PROCS
SEED, OFFSET, ROW_BASE = 0xB10C5EED4321, 9, 3
MARGIN = 0.02           # a steered ratio stays this far from the uniform it is steered against
VOCABS = [37, 2047, 2048, 2049, 4100]
GAMMAS = [1, 2, 4, 32]
BATCHES = [16, 1, 5]
DTYPES = mw.DTYPES
SERVING = (2, 4, 128256, torch.bfloat16, "multinomial", "none", "packed")

# the scenarios a sequence's drafts are steered to (b % len): the iid drafts as drawn; every test fails
# (n = 0); the block stops at depth d, 1 <= d < γ; every draft accepted; every draft accepted with one of
# them the case's stop token; and rescue: the token-wise walk on the same uniforms rejects draft 0, the
# block walk still accepts a deeper draft
SCENARIOS = ("iid", "rej0", "rejD", "full", "stop", "rescue")
# input seeds of the grid's cases for which 11 does not meet what tests/test_block_cpu.py asks of them
# (every scenario reached, no case all close): the lowest seed above 11 that does.  Key: grid()'s tuple
SEEDS = {}


def grid():
    """(B, γ, V, dtype, processor, mask, layout): every V with every γ; batch, dtype and processor
    cycle so that each γ meets every batch size and dtype and each processor every dtype (the keep
    processors on bf16 and fp32 only: the reference's mask value does not fit fp16); every third case
    has `-inf` entries (half of every row), every fourth lies on padded or shifted rows in a poisoned buffer."""
    cases = []
    names = list(PROCS)
    for i, V in enumerate(VOCABS):
        for j, g in enumerate(GAMMAS):
            n = len(cases)
            dtype, name = DTYPES[(i + j) % 3], names[(n + i) % len(names)]
            if dtype == torch.float16 and ("topk" in name or "nucleus" in name):
                name = "multinomial_T0.7" if n % 2 else "greedy"
            if V < 50 and "nucleus" in name:               # a nucleus over 37 tokens keeps one: P == Q, nothing to test
                name = "topk50"
            mask = "half" if n % 3 == 2 else "none"      # ("most" leaves two finite entries: P == Q again)
            layout = rowe.LAYOUTS[1 + (n // 4) % 2] if n % 4 == 1 else "packed"
            cases.append((BATCHES[(i + 2 * j) % 3] if g >= 2 else BATCHES[(i + j) % 3], g, V, dtype, name, mask, layout))
    # every γ >= 2 has a 16-sequence case per dtype that reaches every scenario; the keep processors with them
    cases += [(16, 2, 2049, torch.float32, "topk50", "none", "packed"),
              (16, 4, 4100, torch.bfloat16, "topk50_nucleus0.9", "none", "padded"),
              (16, 32, 2047, torch.bfloat16, "nucleus0.9", "none", "packed"),
              (16, 4, 2048, torch.float16, "multinomial", "half", "shifted"),
              (16, 2, 37, torch.bfloat16, "greedy", "none", "packed"),
              (16, 32, 4100, torch.float32, "multinomial_T0.7", "none", "packed")]
    cases.append(SERVING)
    return cases


def case_id(c):
    B, g, V, dt, name, mask, layout = c
    return f"B{B}-g{g}-V{V}-{str(dt).split('.')[-1]}-{name}-{mask}-{layout}"


def _ratios(P, Q, t):
    q, p = Q[t].astype(np.float64), P[t].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q >= 1e-4, p / q, np.nan)


def _steer(P, Q, tok, scn, uni):
    """Overwrite tok [γ] so that the host walk follows the scenario where the rows and the uniforms
    allow it (what cannot be met with MARGIN leaves the iid draft)."""
    g = len(tok)
    hi = lambda t: int(np.nanargmax(_ratios(P, Q, t)))     # noqa: E731
    lo = lambda t: int(np.nanargmin(_ratios(P, Q, t)))     # noqa: E731
    if any(np.isnan(_ratios(P, Q, t)).all() for t in range(g)) or scn == "iid":
        return
    if scn in ("full", "stop"):
        for t in range(g):
            tok[t] = hi(t)
    elif scn == "rej0":
        tok[0] = lo(0)                                     # w_1 and every later weight stay small
    elif scn == "rejD" and g >= 2:
        d = max(1, g // 2)
        for t in range(d):
            tok[t] = hi(t)
        tok[d] = lo(d)
    elif scn == "rescue" and g >= 2:
        r0 = _ratios(P, Q, 0)
        ok = np.nonzero(r0 < uni[0] - MARGIN)[0]           # token-wise: draft 0 rejected ...
        if len(ok):
            tok[0] = int(ok[np.argmax(r0[ok])])            # ... by the largest such ratio,
            for t in range(1, g):
                tok[t] = hi(t)                             # which the later ratios make up for


@functools.lru_cache(maxsize=8)
def case(B, g, V, dtype, proc_name, mask="none", layout="packed"):
    """Rows tl [B, γ+1, V], dl [B, γ, V] (target logits randn * 3 with `mask`'s `-inf` entries, dl = tl +
    N(0, 0.7²): the same entries at `-inf`), the oracle's rounded probabilities P, Q, drafts tok [B, γ]
    drawn iid from Q and then steered by sequence b's scenario SCENARIOS[b % 6], the stop list (the
    "stop" sequences' draft min(1, γ-1)), the per-depth mass tolerances s_tol [B, γ] and bonus_tol [B]
    (multidraft_ref.MASS_TOL plus multi_walk.flip_slack of the rows) and the host results `rows`."""
    key = (B, g, V, dtype, proc_name, mask, layout)
    seed = SEEDS.get(key, 11)
    gen = torch.Generator().manual_seed(seed * 1000003 + g * 7 + V + B * 131)
    tl = rowe.logits((B, g + 1, V), dtype, seed * 7919 + g * 7 + V + B * 131, mask)
    dl = (tl[:, :g].float() + 0.7 * torch.randn(B, g, V, generator=gen)).to(dtype)
    proc = PROCS[proc_name]
    P = ref.process(tl, proc, exact=True).float()
    Q = ref.process(dl, proc, exact=True).float()
    tok = torch.multinomial(Q.reshape(-1, V), 1, generator=gen).reshape(B, g)
    for b in range(B):
        uni = [float(ph.accept_uniform(SEED, OFFSET, ROW_BASE + b, i)) for i in range(g)]
        t = tok[b].numpy().copy()
        _steer(P[b].numpy(), Q[b].numpy(), t, SCENARIOS[b % len(SCENARIOS)], uni)
        tok[b] = torch.from_numpy(t)
    stops = sorted({int(tok[b, min(1, g - 1)]) for b in range(B) if SCENARIOS[b % len(SCENARIOS)] == "stop"})
    c = SimpleNamespace(B=B, gamma=g, V=V, dtype=dtype, proc=proc, proc_name=proc_name, mask=mask, layout=layout,
                        tl=tl, dl=dl, P=P, Q=Q, tok=tok, stops=stops)
    slack = lambda row: mw._slack_of(c, row)               # noqa: E731
    c.s_tol = [[mref.MASS_TOL + slack(tl[b, t]) + slack(dl[b, t]) for t in range(g)] for b in range(B)]
    c.bonus_tol = [mref.MASS_TOL + slack(tl[b, g]) for b in range(B)]
    c.rows = host_results(c)
    return c


def host_results(c, stops=None, seed=SEED, off=OFFSET, row_base=ROW_BASE):
    """The host model's step of every sequence of case c."""
    stops = c.stops if stops is None else stops
    return [br.philox_step(c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy(), seed, off,
                           row_base + b, stops, greedy=not c.proc.stochastic, s_tol=c.s_tol[b],
                           bonus_tol=c.bonus_tol[b]) for b in range(c.B)]


def coverage(c):
    """What the host walks of a case reached."""
    g = c.gamma
    cov = SimpleNamespace(rej0=0, rej_deep=0, full=0, stop=0, iid=0, rescue=0, close=0)
    for b, r in enumerate(c.rows):
        cov.close += r.close
        cov.rescue += r.rescue
        cov.stop += r.status == br.STOP
        cov.rej0 += r.status == br.RESIDUAL and r.n == 0
        cov.rej_deep += r.status == br.RESIDUAL and 1 <= r.n < g
        cov.full += r.status == br.BONUS
        cov.iid += SCENARIOS[b % len(SCENARIOS)] == "iid"
    return cov


# ---------------------------------------------------------------- the statistical acceptance test's pair
STAT_V, STAT_GAMMA, STAT_B = 8, 4, 16384


@functools.lru_cache(maxsize=1)
def stat_pair(dtype=torch.float32):
    """The context-free pair of the statistical acceptance test: logits tl, dl [V] and the oracle's
    rounded probabilities p, q (fp64), chosen spread out so that block and token-wise expectations differ."""
    g = torch.Generator().manual_seed(77)
    tl = (torch.randn(STAT_V, generator=g) * 1.5).to(dtype)
    dl = (tl.float() + 1.2 * torch.randn(STAT_V, generator=g)).to(dtype)
    proc = PROCS["multinomial"]
    p = ref.process(tl[None], proc, exact=True)[0].double().numpy()
    q = ref.process(dl[None], proc, exact=True)[0].double().numpy()
    return tl, dl, p, q


@functools.lru_cache(maxsize=1)
def stat_expectations():
    """(block E[n], token-wise E[n], standard error of the block mean over STAT_B sequences)."""
    _, _, p, q = stat_pair()
    eb, et, eb2 = br.context_free_expectations(p, q, STAT_GAMMA)
    return eb, et, float(np.sqrt(max(eb2 - eb * eb, 0.0) / STAT_B))


# ---------------------------------------------------------------- the loop on FakeLM banks
def step_rows(target, drafter, prev_token, cur, tok, proc):
    """(P [γ+1, V], Q [γ, V]) of one loop step (multi_walk.step_rows at one chain)."""
    P, Q = mw.step_rows(target, drafter, prev_token, cur, np.asarray(tok)[None], proc)
    return P[0], Q[0]


def simulate_acceptance(target, drafter, g, steps, seed, block=True, proc=None):
    """Mean accepted drafts per step of the block loop (or the token-wise one) on a FakeLM pair, by the
    host model with numpy noise (drafts iid from the exact q): the analogue of
    multi_walk.simulate_acceptance."""
    proc = proc or PROCS["multinomial"]
    rng = np.random.default_rng(seed)
    rows = target.bank.shape[0]
    Pb = ref.process(target.bank.cpu(), proc, exact=True).double().numpy()
    Qb = ref.process(drafter.bank.cpu(), proc, exact=True).double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % rows   # noqa: E731
    prev, cur, total = 3, 8, 0
    V = Pb.shape[1]
    for _ in range(steps):
        tok = np.zeros(g, dtype=np.int64)
        P, Q = np.zeros((g + 1, V)), np.zeros((g, V))
        t = prev
        for d in range(g):
            i = row(t, cur - 1 + d)
            P[d], Q[d] = Pb[i], Qb[i]
            t = tok[d] = rng.choice(V, p=Qb[i] / Qb[i].sum())
        P[g] = Pb[row(t, cur - 1 + g)]
        uni = rng.random(g)
        if block:
            o = br.walk(P, Q, tok, lambda t, h: not (uni[t - 1] > h))
            n, w = o.n, o.weights
        else:
            n = br.tokenwise_n(P, Q, tok, uni)
            w = P[g] if n == g else np.maximum(P[n] - Q[n], 0.0)
        total += n
        prev = rng.choice(V, p=w / w.sum())
        cur += n + 1
    return total / steps
