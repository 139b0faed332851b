"""Host model of the PHILOX (perf) verify, shared by the GPU tests and the CPU tests that prove
their coverage: the accept walks on the numpy Philox uniforms (tests/philox_ref.py), constructed
inputs whose walks reach chosen draft indices, and the chunk an inverse-CDF pick may return.

Everything here runs on the host from the exact-arithmetic oracle (oracle/specdec_ref.py, softmax
in fp64 rounded once to the rows' dtype); no GPU, no library import.  Cases are cached and shared:
callers must not modify the tensors they get.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import philox_ref as ph
from oracle import specdec_ref as ref

MASS_TOL = 1e-5            # the north star's probability-mass tolerance
CHUNK_WIDTH = 2048         # one sampling chunk: kThreads * 8 elements on every verify path
WALK_PROC = ref.Processor("multinomial", 1.0)


def flip_slack(logits_row, dtype):
    """Σ over the row's elements of how far its rounded probability can move when the softmax
    normaliser is off by 1e-6 (relative): the exact fp64 value, scaled by 1 ± 1e-6, rounded to the
    row's dtype both ways."""
    v = torch.softmax(logits_row.double(), dim=-1)
    return float(((v * (1 + 1e-6)).to(dtype).double() - (v * (1 - 1e-6)).to(dtype).double()).sum())


# ---------------------------------------------------------------- accept walk
def host_walk_spec(p, q, seed, off, b, g, uniform=ph.accept_uniform):
    """sampling/speculative_decoding.py:139-145 on Philox uniforms: n, and whether any comparison
    sat within fp32 rounding of the threshold (then the device may legitimately differ).
    uniform(seed, off, b, i): draft i's accept uniform (tests/window_walk.py passes a window's)."""
    n, close = g, False
    for i in range(g):
        r = uniform(seed, off, b, i)
        frac = np.float32(p[i]) / np.float32(q[i]) if q[i] != 0 else np.float32(np.inf if p[i] > 0 else np.nan)
        close |= bool(abs(float(r) - float(frac)) <= 1e-6 * max(1.0, float(frac)))
        if r > frac and n == g:
            n = i
    return n, close


def host_walk_engine(p, q, toks, ends, seed, off, b, g, uniform=ph.accept_uniform):
    """engine/infer_engine.py:297-330 on Philox uniforms: (n, rejected, finished, close)."""
    n, close = 0, False
    for i in range(g):
        u = float(uniform(seed, off, b, i))
        ap = 1.0 if q[i] <= 0 else min(1.0, float(p[i]) / float(q[i]))
        close |= abs(u - ap) <= 1e-6
        if u < ap:
            n += 1
            if int(toks[i]) in ends:
                return n, False, True, close
        else:
            return n, True, False, close
    return n, False, False, close


# ---------------------------------------------------------------- constructed inputs
def pivots(gamma, extra=()):
    """The draft indices edge_walk_case steers walks to: the first and last draft of a Philox block
    of four uniforms (0, 3 | 4, 7 | 8), and the last draft; `extra` adds indices (those below gamma)."""
    return sorted(({0, 3, 4, 7, 8, gamma - 1} | set(extra)) & set(range(gamma)))


def _oracle_probs(tl, dl, gamma):
    """(P [B, γ+1, V], Q [B, γ, V]): the dtype-rounded exact softmaxes of the rows, as fp32."""
    return ref.process(tl, WALK_PROC, exact=True).float(), ref.process(dl, WALK_PROC, exact=True).float()


@functools.lru_cache(maxsize=None)
def _edge(B, gamma, V, dtype, seed, piv=None):
    """piv: the pivot cycle (a tuple, taken in its own order); None: pivots(gamma)."""
    g = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, gamma + 1, V, generator=g) * 3).to(dtype)
    bump = torch.randn(B, gamma, V, generator=g) * 0.5
    piv = pivots(gamma) if piv is None else list(piv)
    k = [piv[b % len(piv)] for b in range(B)]
    dl = tl[:, :gamma].clone()
    for b in range(B):
        dl[b, k[b]:] = (tl[b, k[b]:gamma].float() + bump[b, k[b]:]).to(dtype)
    P, Q = _oracle_probs(tl, dl, gamma)
    ids = torch.empty(B, gamma, dtype=torch.long)
    for b in range(B):
        kb = k[b]
        ids[b, :kb] = tl[b, :kb].float().argmax(-1)
        assert torch.equal(P[b, :kb], Q[b, :kb])
        dist = (P[b, kb:gamma] / Q[b, kb:] - 0.5).abs()
        ids[b, kb:] = dist.masked_fill(~(Q[b, kb:] >= 1e-4), math.inf).argmin(-1)
    return SimpleNamespace(tl=tl, dl=dl, ids=ids, k=k, P=P, Q=Q, B=B, gamma=gamma, V=V, dtype=dtype)


def edge_walk_case(B, gamma, V, dtype, seed):
    """(tl [B, γ+1, V], dl [B, γ, V], ids [B, γ], k [B]): a constructed input whose walk is certain to
    reach the row's pivot index k[b] (cycled over pivots(γ)) and is a coin flip from there on.

    Drafts i < k[b]: dl == tl bit for bit and the draft is the row's argmax, so p == q exactly, the
    ratio is exactly 1, SPEC's r > 1 never rejects and ENGINE's u < 1 always accepts.  Drafts
    i >= k[b]: dl = tl + N(0, 0.5²) and the draft is the token whose exact-oracle ratio p/q is
    nearest 0.5 among the tokens with q >= 1e-4.  Target logits are randn * 3."""
    c = _edge(B, gamma, V, dtype, seed)
    return c.tl, c.dl, c.ids, c.k


@functools.lru_cache(maxsize=None)
def _long(B, gamma, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, gamma + 1, V, generator=g) * 3).to(dtype)
    sigma = torch.tensor([0.04 * (1 + b % 8) for b in range(B)]).view(B, 1, 1)
    dl = (tl[:, :gamma].float() + sigma * torch.randn(B, gamma, V, generator=g)).to(dtype)
    P, Q = _oracle_probs(tl, dl, gamma)
    ids = torch.stack([torch.multinomial(Q[b], 1, generator=torch.Generator().manual_seed(seed * 1000 + b)).squeeze(-1)
                       for b in range(B)])
    return SimpleNamespace(tl=tl, dl=dl, ids=ids, k=None, P=P, Q=Q, B=B, gamma=gamma, V=V, dtype=dtype)


def long_walk_case(B, gamma, V, dtype, seed):
    """(tl, dl, ids): the random bulk case.  dl = tl + sigma_b N(0, 1), sigma_b = 0.04 (1 + b % 8); the
    drafts are drawn from the exact-oracle q by torch.multinomial with a per-row CPU generator."""
    c = _long(B, gamma, V, dtype, seed)
    return c.tl, c.dl, c.ids


def walk_case(kind, B, gamma, V, dtype, seed, piv=None):
    """The cached case with its oracle probabilities: .tl .dl .ids .k .P .Q (kind: "edge" | "long").
    piv: an edge case's own pivot cycle (a tuple; tests/window_walk.py), None: pivots(gamma)."""
    if kind == "edge":
        return _edge(B, gamma, V, dtype, seed) if piv is None else _edge(B, gamma, V, dtype, seed, tuple(piv))
    return _long(B, gamma, V, dtype, seed)


# ---------------------------------------------------------------- chunk pick
def chunk_bracket(weights, u, width=CHUNK_WIDTH, tol=MASS_TOL):
    """(lo, hi), inclusive: the chunks an inverse-CDF pick over `weights` (fp64, non-negative) with the
    uniform u in [0, 1) may return.  Chunk c covers ids [c·width, min(V, (c+1)·width)); the pick is
    the first chunk with positive mass whose running total exceeds u·Σ (the last positive one when
    none does).  lo != hi only when u·Σ lies within tol·Σ of a chunk boundary."""
    w = np.asarray(weights, dtype=np.float64)
    mass = [float(w[c0:c0 + width].sum()) for c0 in range(0, len(w), width)]
    total = math.fsum(mass)
    assert total > 0 and min(mass) >= 0

    def pick(t):
        run, last = 0.0, -1
        for c, m in enumerate(mass):
            run += m
            if m > 0:
                last = c
                if run > t:
                    return c
        return last

    return pick((u - tol) * total), pick((u + tol) * total)


# ---------------------------------------------------------------- a case's host results
def active_mask(B):
    """The ENGINE cases' active rows (as tests/test_gpu_fused.py masks them)."""
    return [b % 5 != 3 for b in range(B)]


def host_rows(case, rule, seed, off, ends=(), row_base=0, active=None):
    """What the oracle and the numpy Philox say of every row of `case` for one verify call with noise
    (seed, off) and global rows row_base + b.  Per row a namespace:
      .active  the row takes part (ENGINE's mask; always True under SPEC)
      .want .close         accepted drafts, and whether a comparison was a close call
      .rejected .finished  (ENGINE) how the walk ended; SPEC: rejected = want < γ
      .cmps    [(i, ratio, accepted)] of the comparisons the walk reached (ratio: p/q, capped at 1
               under ENGINE)
      .slot    the target row the next token is drawn from (None: no token)
      .weights "residual" | "bonus" | "p" | None, .bracket (lo, hi) of chunk_bracket for the row's
               cdf_uniform, .res_mass Σ(p - q)+ of a residual row
    """
    g, ids, P, Q = case.gamma, case.ids, case.P, case.Q
    rows = []
    for b in range(case.B):
        r = SimpleNamespace(active=active is None or bool(active[b]), want=0, close=False, rejected=False,
                            finished=False, cmps=[], slot=None, weights=None, bracket=None, res_mass=None)
        rows.append(r)
        if not r.active:
            continue
        p = [float(P[b, i, ids[b, i]]) for i in range(g)]
        q = [float(Q[b, i, ids[b, i]]) for i in range(g)]
        rb = row_base + b
        if rule == "spec":
            r.want, r.close = host_walk_spec(p, q, seed, off, rb, g)
            r.rejected = r.want < g
            reached = min(r.want, g - 1)
            ratio = [p[i] / q[i] for i in range(g)]
        else:
            r.want, r.rejected, r.finished, r.close = host_walk_engine(p, q, ids[b], ends, seed, off, rb, g)
            reached = r.want if r.rejected else r.want - 1
            ratio = [min(1.0, p[i] / q[i]) for i in range(g)]
        r.cmps = [(i, ratio[i], i < r.want) for i in range(reached + 1)]
        if r.rejected:
            w = (P[b, r.want].double() - Q[b, r.want].double()).clamp(min=0)
            r.slot, r.weights, r.res_mass = r.want, "residual", float(w.sum())
            if rule == "engine" and r.res_mass <= 1e-12:      # engine/infer_engine.py:319-321
                w, r.weights = P[b, r.want].double(), "p"
        elif rule == "spec":
            w = P[b, g].double()
            r.slot, r.weights = g, "bonus"
        if r.weights is not None:
            r.bracket = chunk_bracket(w.numpy(), ph.cdf_uniform(seed, off, rb))
    return rows


def late_end(case, rows, min_index=4):
    """(row, index) of an accepted draft at index >= min_index of an active row (host walk `rows`,
    run without end tokens): ends that hold this draft's token finish the row from a late draft.
    None when there is none."""
    for b, r in enumerate(rows):
        for i in range(min_index, r.want):
            return b, i
    return None


def engine_ends(case, seed, off, row_base=0, active=None):
    """The ENGINE cases' end tokens: a late accepted draft's token (late_end, γ >= 5) and row 0's
    first draft.  Returns (ends, late) with late = (row, index) or None."""
    free = host_rows(case, "engine", seed, off, (), row_base, active)
    late = late_end(case, free) if case.gamma >= 5 else None
    ends = [int(case.ids[0, 0])]
    if late is not None:
        ends.insert(0, int(case.ids[late[0], late[1]]))
    return ends, late


def coverage(case, rows):
    """Counts over the comparisons the host walks reached: what keeps a GPU test from passing
    vacuously.  mid = ratio in [0.1, 0.9]."""
    c = SimpleNamespace(pivot_mid={}, acc4=0, rej4=0, acc8=0, rej8=0, mid4=0, close=0, full=0, early_rej=0, widened=0)
    g = case.gamma
    for r in rows:
        if not r.active:
            continue
        c.close += r.close
        c.full += (not r.rejected) and r.want == g
        c.early_rej += r.rejected and r.want < 4
        c.widened += r.bracket is not None and r.bracket[0] != r.bracket[1]
        for i, ratio, acc in r.cmps:
            mid = 0.1 <= ratio <= 0.9
            if mid:
                c.pivot_mid[i] = c.pivot_mid.get(i, 0) + 1
            if i >= 4:
                c.mid4 += mid
                c.acc4 += acc
                c.rej4 += not acc
            if i >= 8:
                c.acc8 += acc
                c.rej8 += not acc
    return c
