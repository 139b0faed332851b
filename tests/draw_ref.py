"""Host model of the three PHILOX draw kernels of sd_sample — k_draw, k_draw_lean
(csrc/specdec_kernels.hip) and k_draw_nuc (csrc/sd_draw_nucleus.inc) — in fp64 numpy over the numpy
Philox (tests/philox_ref.py), and the checker that holds a device token to it.

A draw is a pure function of (row values, seed, offset, global row).  Every kernel draws in two levels:
each span (k_draw_nuc: slice) draws its own candidate by inverse CDF over its weights, walked in a
fixed element order, on a uniform of its own; the row then picks one span and returns that span's
candidate.

Element order.  A span of NST stages keeps EPT = NST·VEC elements per thread (VEC = 8 for 16-bit rows, 4
for fp32; 256 threads) and its running sum goes in (thread, k) order: position tid·EPT + k is element
base + ((k // VEC)·256 + tid)·VEC + k % VEC (chunk_elem).  Elements at or past V carry weight 0.  A
k_draw_nuc slice is 2048 elements in linear order.

  k_draw        y = process_value(x) in the row dtype (keep predicate as the call's row_keep_out gives
                it, then round_dt(y / T)); span c: m_c = max y, w = exp(y - m_c), candidate by inverse
                CDF on cdf_uniform(row, 1 + c); the row: inverse CDF over W_c = S_c·exp(m_c - M) on
                cdf_uniform(row, 0).  nst = 1 while B·ceil(V / 2048) <= 1024, else 2; fp32: 2 stages of
                1024 elements.
  k_draw_lean   the same candidates over the raw 16-bit values; the span is argmax_c (m_c + ln S_c + g_c)
                with g_c = span_gumbel(row, c), the lowest c on an exact tie; spans with S_c = 0 or
                m_c = -inf do not race.  NST = 1 for B <= 128, 4 above (SD_OPT_DRAW_SPAN pins it).
  k_draw_nuc    rounds 0..7 of proposals k = 0..3, uniform index base 128·(4·round + k): base + 0 picks
                the slice over S'_c·exp(my_c - MY), base + 1 + c slice c's element over exp(y - my_c),
                y = round_dt(x / T).  Proposal j is kept iff round_dt(A_j) <= round_dt(top_p), A_j the
                T = 1 mass p = round_dt(exp(x - M) / s) of the elements strictly before j (a larger
                value, or an equal value at a lower index).  The token is the first kept proposal.

Tolerances — each from the device arithmetic as the kernels write it, none fitted to an output.
EPS = 2^-24 is the unit roundoff of fp32 (half an ulp, relative).

  W_RTOL = 2^-22 per unit of (1 + |y - m|): a weight is exp2((y - m)·log2e) — y - m is exact (16-bit
      operands, or one fp32 subtraction: EPS), the multiply by the rounded log2e adds EPS·|y - m|·log2e to
      the argument, i.e. EPS·|y - m| relative to the result, and the hardware exp2 is good to about an ulp
      (2·EPS).  k_draw_lean forms the same weight as exp2((y - m_w)·log2e)·exp2((m_w - m)·log2e) with m_w
      its wave's maximum: two exps and a product, (|y - m_w| + |m_w - m|) = |y - m|, under 4·EPS·(1 + |y - m|)
      in all.  So slack_w = Σ_j w_j·(1 + |y_j - m_c|)·2^-22 bounds what the weights' own rounding moves any
      running total of the span.
  k_draw / k_draw_nuc add the fp32 weights exactly in fp64 (chunk_pick; 2048 terms of 53-bit sums: 2^-42
      relative, nothing beside slack_w): the in-span slack is slack_w.  k_draw's aligned 16-bit T = 1
      branch (chunk_pick_tot) first adds each thread's EPT weights in fp32: EPT roundings of at most EPS
      of the thread's total each, + EPT·EPS·T_c.
  k_draw_lean adds in fp32 throughout: the thread's sequential total (EPT roundings), the 6-step wave scan,
      the 4 wave offsets, the fma that rescales the lane's prefix (counted with the offsets: 4) and one
      fma per element in the claiming lane's walk (EPT more): + (2·EPT + 6 + 4 + 4)·EPS·T_c.
  Span pick of k_draw (and the slice pick of k_draw_nuc): the fp64 scan of W_c = fl(fl(S_c)·sd_exp(m_c - M));
      fl(S_c) and the product round once each (2·EPS) and sd_exp is good to 2·EPS·(1 + |m_c - M|) (its
      argument carries a compensated log2e): slack_W = Σ_c W_c·(1 + |m_c - M|)·2^-22.
  Span race of k_draw_lean: key_c = fl(fl(m_c + __logf(S_c)) + g_c), g_c = -__logf(E_c), E_c = -__logf(u_c).
      __logf is the hardware log2 times ln 2: about 2 ulp of its result, but for an argument next to 1 the
      error is absolute, so each logarithm is charged 4·EPS·max(1, |result|).  E_c's error reaches g_c
      as a relative one: 4·EPS·max(1, 1 / E_c) (absolute on g_c = -ln E_c; it only grows where u_c lies
      within about 2^-20 of 1).  The two additions round once each: EPS·(|m_c + ln S_c| + |key_c|).  And
      the device's S_c is the fp32 total the in-span slack describes: slack_c / T_c on ln S_c.  So
        tol_c = EPS·(4·max(1, |ln S_c|) + 4·max(1, |g_c|) + |m_c + ln S_c| + |key_c|)
                + 4·EPS·max(1, 1 / E_c) + slack_c / T_c,
      and two spans compare within tol_a + tol_b.
  k_draw_nuc's keep test: the device forms p from an fp32 exp, the fp32 normaliser and a division; the
      suite holds such a probability to P_RTOL = 2e-6 relative (tests/test_gpu_row_edges.py, and
      kCutSlackF32 in csrc/sd_threshold.inc is the same figure for the same sum).  The model carries
      A_j three times — over round_dt(p), round_dt(p·(1 - P_RTOL)) and round_dt(p·(1 + P_RTOL)) — and a
      proposal whose keep decision differs between the outer two is a close call.

SLACK_CAP: every in-span slack stays under 1e-5·T_c and every span-pick slack under 1e-5·ΣW
(tests/test_draw_ref_cpu.py asserts it for every case of tests/draw_cases.py).  CLOSE_CAP: at most
2 % of a case's rows may be close calls of any kind; each must still pass its interval or key test.
A close call is a row whose device token differs from the model's (an inverse-CDF pick on the other side
of an edge), a row whose two best race keys lie within tol of each other, or a row with a close keep
decision.  The models say so themselves: `close` (race keys, keep decisions) and `edge` (a CDF target
within the slack of an edge of its element's or span's interval) — a differing token without either
flag fails.

Test infrastructure only: no GPU, no library import.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import philox_ref as ph

THREADS = 256
EPS = 2.0 ** -24
W_RTOL = 2.0 ** -22
P_RTOL = 2e-6
SLACK_CAP = 1e-5
CLOSE_CAP = 0.02
NEG_FILL = -1e20                 # sd_device.h kNegFill
TINY = 2.0 ** -150               # below half the smallest fp32 denormal: the device's fp32 weight is 0
NUC_K, NUC_ROUNDS, NUC_SLICE = 4, 8, 2048
LEAN_SPAN4_MIN_B = 128           # specdec_kernels.hip kDrawSpan4MinB


# ---------------------------------------------------------------- formats
def vec_of(dtype) -> int:
    return 4 if dtype == torch.float32 else 8


def round32(a, dtype):
    """fp32 array -> dtype -> fp32 (round_dt of the kernels), as a numpy fp32 array."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if dtype == torch.float32:
        return a
    return torch.from_numpy(a).to(dtype).float().numpy()


def round64(a, dtype):
    """fp64 -> fp32 -> dtype, back in fp64 (the device rounds an fp32 value to the row dtype)."""
    with np.errstate(over="ignore", under="ignore"):
        a32 = np.asarray(a, dtype=np.float64).astype(np.float32)
    return round32(a32, dtype).astype(np.float64)


def values32(x):
    """A row tensor's values as a numpy fp32 array (exact for every row dtype)."""
    return x.detach().cpu().float().numpy()


def processed(x, dtype, temperature=1.0, keep=None):
    """process_value (sd_device.h) over the row x: the keep predicate (tau, tie_idx) — x > tau, or x == tau
    and j <= tie_idx; the rest becomes round_dt(-1e20) — then round_dt(v / T) by an fp32 division.  fp64 [V]."""
    v = values32(x).copy()
    if keep is not None:
        tau, tie = np.float32(keep[0]), int(keep[1])
        kept = (v > tau) | ((v == tau) & (np.arange(len(v)) <= tie))
        v = np.where(kept, v, round32([NEG_FILL], dtype)[0]).astype(np.float32)
    if temperature != 1.0:
        with np.errstate(over="ignore"):
            v = round32(v / np.float32(temperature), dtype)
    return v.astype(np.float64)


def keep_of(rec):
    """(tau, tie_idx, flags) of one sd_row_keep record (int32 [4]: tau's fp32 bits, tie index, flags)."""
    r = np.asarray(rec, dtype=np.int32)
    return float(r[0:1].view(np.float32)[0]), int(r[1]), int(r[2])


# ---------------------------------------------------------------- element order
def span_order(nst: int, vec: int):
    """Element offsets inside a span in the order its running sum goes: position tid·EPT + k ->
    ((k // VEC)·256 + tid)·VEC + k % VEC (the inverse of chunk_elem)."""
    ept = nst * vec
    pos = np.arange(THREADS * ept)
    tid, k = pos // ept, pos % ept
    return ((k // vec) * THREADS + tid) * vec + k % vec


def linear_order(nst: int, vec: int):
    return np.arange(THREADS * nst * vec)


# ---------------------------------------------------------------- spans
def span_tables(y, nst: int, vec: int, order=span_order, extra_ulps: int = 0):
    """The spans of the processed row y (fp64 [V], -inf allowed): per span its elements in walk order (idx,
    those below V), their weights w = exp(y - m) and running totals cum, m, T = Σw and the in-span slack
    Σ w·(1 + |y - m|)·2^-22 + extra_ulps·EPS·T."""
    y = np.asarray(y, dtype=np.float64)
    V, span = len(y), THREADS * nst * vec
    offs = order(nst, vec)
    out = []
    for c in range((V + span - 1) // span):
        idx = c * span + offs
        idx = idx[idx < V]
        yc = y[idx]
        m = float(yc.max())
        if m > -math.inf:
            with np.errstate(invalid="ignore", under="ignore"):
                d = m - yc
                w = np.exp(-d)
            w[w < TINY] = 0.0
            with np.errstate(invalid="ignore"):
                sw = float(np.where(w > 0, w * (1.0 + d), 0.0).sum())
        else:
            w, sw = np.zeros(len(idx)), 0.0
        cum = np.cumsum(w)
        T = float(cum[-1])
        out.append(SimpleNamespace(c=c, base=c * span, idx=idx, w=w, cum=cum, m=m, T=T,
                                   slack=sw * W_RTOL + extra_ulps * EPS * T))
    return out


def pick(cum, u: float) -> int:
    """Inverse CDF: the first position whose running total exceeds u·Σ (it has positive weight: the
    total moved there); the last positive one when rounding runs past the end; -1 without mass."""
    T = float(cum[-1])
    if not T > 0:
        return -1
    p = int(np.searchsorted(cum, u * T, side="right"))
    if p >= len(cum):
        p = int(np.searchsorted(cum, T, side="left"))   # the first position that reaches Σ: the last positive one
    return p


def interval(cum, p: int):
    """(lo, hi) of position p: the running total before and after it."""
    return (float(cum[p - 1]) if p > 0 else 0.0), float(cum[p])


def near_edge(cum, p: int, t: float, slack: float) -> bool:
    """The target t lies within the slack of an edge it shares with another element (not the ends 0 and Σ)."""
    lo, hi = interval(cum, p)
    return (lo > 0 and t - lo <= slack) or (hi < float(cum[-1]) and hi - t <= slack)


def excess(cum, p: int, t: float) -> float:
    """How far the target t lies outside position p's interval [lo, hi) (0 inside)."""
    lo, hi = interval(cum, p)
    return lo - t if t < lo else (t - hi if t >= hi else 0.0)


def element_used(span, j: int, t: float) -> float:
    """The in-span interval test of element j against the target t: the share of the span's slack the
    device's pick uses (0: t inside j's interval; <= 1 passes); inf if j is not a positive-weight
    element of the span."""
    at = np.nonzero(span.idx == j)[0]
    if len(at) == 0 or not span.w[at[0]] > 0:
        return math.inf
    e = excess(span.cum, int(at[0]), t)
    return 0.0 if e == 0.0 else (e / span.slack if span.slack > 0 else math.inf)


# ---------------------------------------------------------------- k_draw
def draw_nst(B: int, V: int, dtype) -> int:
    if dtype == torch.float32:
        return 2
    return 1 if B * ((V + 2047) // 2048) <= 1024 else 2


def draw_tables(x, dtype, temperature, keep, nst, order=span_order):
    """k_draw's spans of the row x and the row-level weights W_c = S_c·exp(m_c - M)."""
    y = processed(x, dtype, temperature, keep)
    vec = vec_of(dtype)
    lean_branch = temperature == 1.0 and keep is None and dtype != torch.float32   # chunk_pick_tot
    spans = span_tables(y, nst, vec, order, extra_ulps=nst * vec if lean_branch else 0)
    m = np.array([s.m for s in spans])
    S = np.array([s.T for s in spans])
    M = float(m.max())
    with np.errstate(invalid="ignore"):
        dm = np.where(S > 0, M - m, 0.0)
        W = np.where(S > 0, S * np.exp(-dm), 0.0)
    cumW = np.cumsum(W)
    return SimpleNamespace(kernel="k_draw", y=y, spans=spans, span_len=THREADS * nst * vec, m=m, S=S, M=M, W=W,
                           cumW=cumW, total=float(cumW[-1]), slackW=float((W * (1.0 + dm)).sum()) * W_RTOL)


def draw_decide(tb, u):
    """The draw given its uniforms u [1 + spans] (u[0] the row's, u[1 + c] span c's)."""
    cand, targets, edge = [], [], False
    for c, s in enumerate(tb.spans):
        p = pick(s.cum, float(u[1 + c]))
        cand.append(int(s.idx[p]) if p >= 0 else -1)
        targets.append(float(u[1 + c]) * s.T)
    span = pick(tb.cumW, float(u[0]))
    row_target = float(u[0]) * tb.total
    token = cand[span] if span >= 0 else -1
    if span >= 0:
        s = tb.spans[span]
        edge = near_edge(tb.cumW, span, row_target, tb.slackW) or \
            near_edge(s.cum, int(np.nonzero(s.idx == token)[0][0]), targets[span], s.slack)
    return SimpleNamespace(u=u, cand=cand, targets=targets, row_target=row_target, span=span, token=token, edge=edge,
                           close=False)


def draw_row(tb, seed, off, grow, uniform=ph.cdf_uniform):
    return draw_decide(tb, np.atleast_1d(uniform(seed, off, grow, np.arange(len(tb.spans) + 1, dtype=np.uint64))))


def token_prob(tb, tok: int, dtype):
    """round_dt of the fp64 processed probability of tok."""
    with np.errstate(invalid="ignore", under="ignore"):
        S = float(np.where(tb.y > -math.inf, np.exp(tb.y - tb.M), 0.0).sum())
        return float(round64([math.exp(tb.y[tok] - tb.M) / S], dtype)[0])


def check_draw(tb, r, tok: int):
    """The device's token against the model r of the same (seed, offset, row): (ok, close, used, why).
    Equal to the model's token; or its span passes the interval test over the W_c and the token the
    in-span one (a close call).  used: the largest share of a slack the device's pick needed."""
    if tok == r.token and tok >= 0:
        return True, False, 0.0, ""
    if not 0 <= tok < len(tb.y):
        return False, False, math.inf, f"token {tok} outside the row (model {r.token})"
    d = tok // tb.span_len
    if not tb.W[d] > 0:
        return False, False, math.inf, f"span {d} has no mass"
    e = excess(tb.cumW, d, r.row_target)
    used_s = 0.0 if e == 0.0 else e / tb.slackW
    used_e = element_used(tb.spans[d], tok, r.targets[d])
    used = max(used_s, used_e)
    why = (f"token {tok} (span {d}) model {r.token} (span {r.span}): span slack used {used_s:.3g}, "
           f"in-span slack used {used_e:.3g}")
    return used <= 1.0, True, used, why


# ---------------------------------------------------------------- k_draw_lean
def lean_nst(B: int, pinned: int = 0) -> int:
    return pinned if pinned else (1 if B <= LEAN_SPAN4_MIN_B else 4)


def lean_tables(x, dtype, nst, order=span_order):
    assert dtype != torch.float32
    y = values32(x).astype(np.float64)
    spans = span_tables(y, nst, 8, order, extra_ulps=2 * nst * 8 + 6 + 4 + 4)
    m = np.array([s.m for s in spans])
    S = np.array([s.T for s in spans])
    racing = (S > 0) & (m > -math.inf)
    with np.errstate(divide="ignore"):
        lnS = np.where(racing, np.log(np.where(racing, S, 1.0)), 0.0)
    rel = np.array([s.slack / s.T if s.T > 0 else 0.0 for s in spans])
    return SimpleNamespace(kernel="k_draw_lean", y=y, spans=spans, span_len=THREADS * nst * 8, m=m, S=S, lnS=lnS,
                           racing=racing, rel=rel)


def lean_decide(tb, u, g, E, race=True):
    """The draw given span c's uniform u[c], Gumbel noise g[c] and its E[c]."""
    cand, targets = [], []
    for c, s in enumerate(tb.spans):
        p = pick(s.cum, float(u[c]))
        cand.append(int(s.idx[p]) if p >= 0 else -1)
        targets.append(float(u[c]) * s.T)
    g, E = np.asarray(g, dtype=np.float64), np.asarray(E, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        base = np.where(tb.racing, tb.m, 0.0) + tb.lnS
        keys = np.where(tb.racing, base + g, -math.inf)
        tol = EPS * (4 * np.maximum(1, np.abs(tb.lnS)) + 4 * np.maximum(1, np.abs(g)) + np.abs(base) + np.abs(keys)) \
            + 4 * EPS * np.maximum(1, 1 / E) + tb.rel
        tol = np.where(tb.racing & np.isfinite(keys), tol, 0.0)
    span = int(np.argmax(keys)) if keys.max() > -math.inf else -1     # the lowest c on an exact tie
    token = cand[span] if span >= 0 else -1
    close, edge, gap = False, False, math.inf
    if span >= 0:
        others = np.delete(np.arange(len(keys)), span)
        if len(others) and np.isfinite(keys[span]):
            gaps = keys[span] - keys[others]
            close = bool((gaps <= tol[span] + tol[others]).any())
            gap = float(gaps.min())
        s = tb.spans[span]
        edge = near_edge(s.cum, int(np.nonzero(s.idx == token)[0][0]), targets[span], s.slack)
    return SimpleNamespace(u=u, g=g, E=E, cand=cand, targets=targets, keys=keys, tol=tol, span=span, token=token,
                           close=close, edge=edge, gap=gap)


def lean_row(tb, seed, off, grow, uniform=ph.cdf_uniform, gumbel=ph.span_gumbel):
    c = np.arange(len(tb.spans), dtype=np.uint64)
    g, E = gumbel(seed, off, grow, c)
    return lean_decide(tb, np.atleast_1d(uniform(seed, off, grow, c + np.uint64(1))), np.atleast_1d(g), np.atleast_1d(E))


def check_lean(tb, r, tok: int):
    """(ok, close, used, why): the token's span must have a host key within tol of the best one, and the
    token must be that span's candidate or pass the in-span interval test (a close call)."""
    if tok == r.token and tok >= 0:
        return True, r.close, 0.0, ""
    if not 0 <= tok < len(tb.y):
        return False, False, math.inf, f"token {tok} outside the row (model {r.token})"
    d = tok // tb.span_len
    if not tb.racing[d]:
        return False, False, math.inf, f"span {d} is out of the race"
    used_k = 0.0
    if d != r.span:
        room = float(r.tol[d] + r.tol[r.span])
        used_k = float(r.keys[r.span] - r.keys[d]) / room if room > 0 else math.inf
    used_e = 0.0 if tok == r.cand[d] else element_used(tb.spans[d], tok, r.targets[d])
    used = max(used_k, used_e)
    why = (f"token {tok} (span {d}) model {r.token} (span {r.span}): key gap {float(r.keys[r.span] - r.keys[d]):.3g} "
           f"of tol {float(r.tol[d] + r.tol[r.span]):.3g}, in-span slack used {used_e:.3g}")
    return used <= 1.0, True, used, why


# ---------------------------------------------------------------- k_draw_nuc
def nuc_tables(x, dtype, temperature, top_p):
    assert dtype != torch.float32
    x32 = values32(x)
    x64 = x32.astype(np.float64)
    V = len(x64)
    y = x64 if temperature == 1.0 else round32(x32 / np.float32(temperature), dtype).astype(np.float64)
    slices = span_tables(y, 1, 8, linear_order)
    my = np.array([s.m for s in slices])
    Sc = np.array([s.T for s in slices]).astype(np.float32).astype(np.float64)    # the record carries (float)T_c
    MY = float(my.max())
    ok = (Sc > 0) & (my > -math.inf)
    with np.errstate(invalid="ignore"):
        dm = np.where(ok, MY - my, 0.0)
        W = np.where(ok, Sc * np.exp(-dm), 0.0)
    cumW = np.cumsum(W)
    # the T = 1 probabilities as thr_decide forms them, and the mass strictly before every element
    M = float(x64.max())
    with np.errstate(under="ignore"):
        e = np.exp(x64 - M)
    pe = e / e.sum()
    order = np.argsort(-x64, kind="stable")           # a larger value first, an equal one at the lower index first

    def before(p):
        cs = np.cumsum(p[order])
        A = np.empty(V)
        A[order] = cs - p[order]
        return A

    tpd = float(round32([np.float32(top_p)], dtype)[0])

    def kept(A):
        return round64(A, dtype) <= tpd

    A = before(round64(pe, dtype))
    k_mid = kept(A)
    k_lo = kept(before(round64(pe * (1 - P_RTOL), dtype)))      # the most the device can keep
    k_hi = kept(before(round64(pe * (1 + P_RTOL), dtype)))      # the least
    return SimpleNamespace(kernel="k_draw_nuc", y=y, slices=slices, span_len=NUC_SLICE, W=W, cumW=cumW,
                           total=float(cumW[-1]), slackW=float((W * (1.0 + dm)).sum()) * W_RTOL, A=A, kept=k_mid,
                           sure=k_hi, maybe=k_lo & ~k_hi, pe=pe, top_p=tpd)


def nuc_proposals(tb, seed, off, grow, uniform=ph.nuc_uniform):
    """The row's proposals in round order, then k order (lazily: a Philox call each)."""
    n = len(tb.slices)
    for rnd in range(NUC_ROUNDS):
        for k in range(NUC_K):
            base = 128 * (NUC_K * rnd + k)
            u = np.atleast_1d(uniform(seed, off, grow, np.uint64(base) + np.arange(n + 1, dtype=np.uint64)))
            c = pick(tb.cumW, float(u[0]))
            if c < 0:
                return
            s = tb.slices[c]
            p = pick(s.cum, float(u[1 + c]))
            j = int(s.idx[p])
            yield SimpleNamespace(round=rnd, k=k, slice=c, token=j, u=u, row_target=float(u[0]) * tb.total,
                                  target=float(u[1 + c]) * s.T, kept=bool(tb.kept[j]), sure=bool(tb.sure[j]),
                                  maybe=bool(tb.maybe[j]),
                                  edge=near_edge(tb.cumW, c, float(u[0]) * tb.total, tb.slackW) or
                                  near_edge(s.cum, p, float(u[1 + c]) * s.T, s.slack))


def nuc_row(tb, seed, off, grow, uniform=ph.nuc_uniform):
    """token: the first kept proposal (None: none in 8 rounds — the device flags such a row); accept: the
    tokens the device may return — the model's, and under a close keep decision either outcome's; live:
    the proposals that can be the returned one; rounds: how many rounds the model needed."""
    token, rounds, accept, live, close, edge = None, 0, [], [], False, False
    for q in nuc_proposals(tb, seed, off, grow, uniform):
        if token is None and q.kept:
            token, rounds = q.token, q.round + 1
        if q.sure or q.maybe:
            accept.append(q.token)
            live.append(q)
            close, edge = close or q.maybe, edge or q.edge
        if q.sure:
            break
    return SimpleNamespace(token=token, rounds=rounds, accept=accept, live=live, close=close, edge=edge,
                           first_k=live[0].k if live else None)


def check_nuc(tb, r, tok: int):
    """(ok, close, used, why): tok is one of the tokens the model accepts (one only unless a keep decision
    is close), or it passes the slice and in-slice interval tests on one of the live proposals' uniforms."""
    if r.token is None:
        return False, False, math.inf, "the model kept no proposal in 8 rounds"
    if tok in r.accept:
        return True, r.close, 0.0, ""
    if not 0 <= tok < len(tb.y):
        return False, False, math.inf, f"token {tok} outside the row (model {r.token})"
    d = tok // NUC_SLICE
    best = math.inf
    if tb.W[d] > 0 and (tb.sure[tok] or tb.maybe[tok]):
        for q in r.live:
            e = excess(tb.cumW, d, q.row_target)
            used_s = 0.0 if e == 0.0 else e / tb.slackW
            best = min(best, max(used_s, element_used(tb.slices[d], tok, float(q.u[1 + d]) * tb.slices[d].T)))
    return best <= 1.0, True, best, f"token {tok} model {r.token} accept {r.accept}: slack used {best:.3g}"


# ---------------------------------------------------------------- the slack cap
def slack_shares(tb):
    """(largest in-span slack / T_c, span-pick slack / ΣW) of a row's tables: both stay under SLACK_CAP."""
    spans = tb.spans if hasattr(tb, "spans") else tb.slices
    inner = max((s.slack / s.T for s in spans if s.T > 0), default=0.0)
    outer = tb.slackW / tb.total if hasattr(tb, "slackW") and tb.total > 0 else 0.0
    return inner, outer
