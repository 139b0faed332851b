"""Host model of sd_ngram_verify under SD_NOISE_PHILOX (csrc/sd_ngram.inc, sd_device.h), one step and
a chunked window of γ' > 32 drafts, from the exact-arithmetic oracle and the numpy Philox.

* Segment s of global row rb, element j: word j & 3 of philox_ref.block(seed, off, rb, 8 + s, j >> 2)
  gives u = (w >> 8)·2^-24 + 2^-25 and E = -ln u (philox_ref.exp1_words).
* A draw from processed probabilities p is argmax_j p_j / E_j, lowest index on equality; under greedy
  it is the argmax of p and no noise is read.  p is the oracle's ref.process(..., stable_ties=True,
  exact=True) (fp16 rows under a top-k / nucleus keep: processed in fp32, whose -1e20 fill fp16 lacks).
* Row i < γ' compares its draw on segment i with draft i; n is the first mismatch.  x is a second draw
  from row n on segment n + 1, or from the bonus row on segment γ'.  Stops, stop_index, prune_target and
  the status bits follow k_ngram_finalize (ngram_assisted.py:111-164).
* A window of γ' > 32 drafts: chunk k (drafts [32k, 32k + g_k)) draws with offset off + k and counts
  its segments from 0, so draft i compares on (off + i // 32, segment i % 32) and x is drawn on
  (off + n // 32, segment n % 32 + 1), or for n = γ' on the last chunk's (offset, segment g_k).  The model
  states this for the whole window; it does not import specdec_amd.chunked.

Close draws.  The device computes round_dt(p / round_dt(E)) with E from the fp32 fast logarithm: two
roundings (<= 2^-8 relative in bf16) and the logarithm's error, which no test of this project measures;
an absolute error of the order of 2^-22 would be under 1 % of a winner's E of 5e-5 and reach TAU only below
E ~ 4e-6 (the smallest winner E over the GPU cases is 1.07e-6; every row of an MI355X run equalled the
model).  A draw is therefore flagged close when the runner-up's score is within TAU = 2^-4
(relative) of the winner's, and the tests choose Philox offsets at which no draw that the walks reach is
close (quiet_offset): TAU is a condition on the inputs, not a tolerance on the kernel.
"""
import dataclasses
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import philox_ref as ph
import row_edges as re_
from oracle import specdec_ref as ref

M = 32                                  # SD_MAX_GAMMA
SITE_NGRAM = 8                          # kSiteNgram
TAU = 2.0 ** -4
GREEDY_TAU = 1e-5                       # an argmax between two distinct probabilities closer than fp32 rounding tells
DONE, STOP_IN_DRAFTS, FINISHED, BONUS, FALLBACK_P = 0x1, 0x2, 0x4, 0x10, 0x20
OFFSET = 20                             # where quiet_offset starts
NOISE_SEED = 0xC0FFEE_1234
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
KINDS = {k: re_.KINDS[k] for k in ("greedy", "multi_t1", "multi_t07", "topk20", "nucleus09")}


# ---------------------------------------------------------------- draws
def draw(p, E):
    """(token, relative gap between the top two scores, the winner's E) of argmax_j p_j / E_j."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(p > 0, p / E, 0.0)
    j = int(np.argmax(s))                # first maximum
    rest = np.delete(s, j)
    second = float(rest.max()) if rest.size else 0.0
    gap = 1.0 - second / s[j] if np.isfinite(s[j]) and s[j] > 0 else 0.0
    return j, float(gap), float(E[j])


def draw_greedy(p):
    j = int(np.argmax(p))
    rest = np.delete(p, j)
    second = float(rest.max()) if rest.size else 0.0
    gap = 1.0 - second / p[j]
    return j, (math.inf if gap == 0.0 or gap >= GREEDY_TAU else gap), math.inf


def ngram_rows(P, drafts, stoch, seed, off, row_base=0, stops=()):
    """The step (γ' <= 32) or window (γ' > 32) result of every row.  P: fp64 [B, γ'+1, V] processed
    probabilities, drafts: [B, γ'] ints.  Per row a namespace: .n .x .stop_index .prune_target .status,
    .close (a draw the walk reached was close), .min_gap .min_E over those draws."""
    B, g = P.shape[0], P.shape[1] - 1
    V = P.shape[2]
    rows = []
    for b in range(B):
        rb = row_base + b
        r = SimpleNamespace(n=g, x=-1, stop_index=-1, prune_target=0, status=DONE, close=False, min_gap=math.inf,
                            min_E=math.inf)
        rows.append(r)

        def one(row, k, seg):
            if stoch:
                j, gap, e = draw(P[b, row], ph.exp1_words(seed, off + k, rb, SITE_NGRAM + seg, V)[0])
                r.close |= gap < TAU
            else:
                j, gap, e = draw_greedy(P[b, row])
                r.close |= gap < GREEDY_TAU
            r.min_gap, r.min_E = min(r.min_gap, gap), min(r.min_E, e)
            return j

        for i in range(g):
            if one(i, i // M, i % M) != int(drafts[b][i]):
                r.n = i
                break
        r.stop_index = ref.stop_location(drafts[b][:r.n], stops)
        if r.stop_index >= 0:
            r.status |= STOP_IN_DRAFTS
            continue
        if r.n < g:
            r.x = one(r.n, r.n // M, r.n % M + 1)
            r.status |= FALLBACK_P
            r.prune_target = g - r.n + 1
        else:
            k = max(0, (g - 1) // M)
            r.x = one(g, k, g - k * M)
            r.status |= BONUS
        if r.x in [int(s) for s in stops]:
            r.status |= FINISHED
    return rows


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def ngram_case(B, g, V, dtype, seed, odds=4.0, late_odds=None, plan=None):
    """Peaked rows: randn * 3 logits with one hot token per row whose logit is ln(odds · Σ_others e^x), so
    that it has probability odds / (1 + odds) under multinomial T = 1 (rows from draft 31 on: late_odds).
    The bonus row has no hot token.  Draft i is the hot token of row i, except at the row's planned
    mismatch plan[b % len(plan)] (None: no planned mismatch), where it is the next token id."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, g + 1, V, generator=gen) * 3
    hot = torch.randint(0, V, (B, g + 1), generator=gen)
    for b in range(B):
        for i in range(g):
            o = late_odds if late_odds is not None and i >= M - 1 else odds
            x[b, i, hot[b, i]] = -math.inf
            x[b, i, hot[b, i]] = math.log(o) + float(torch.logsumexp(x[b, i].double(), 0))
    x = x.to(dtype)
    plan = (None, 0, g // 2, None, g - 1) if plan is None else plan
    drafts = hot[:, :g].clone()
    planned = [plan[b % len(plan)] for b in range(B)]
    for b, m in enumerate(planned):
        if m is not None and m < g:
            drafts[b, m] = (drafts[b, m] + 1) % V
    return SimpleNamespace(x=x, drafts=drafts, hot=hot, planned=planned, B=B, gamma=g, V=V, dtype=dtype)


def probs(x, kind):
    """The oracle's processed probabilities of rows x [..., V] in x's dtype (fp16 under a keep: via fp32)."""
    proc = dataclasses.replace(KINDS[kind], stable_ties=True)
    if x.dtype == F16 and proc.kind in re_.KEEP_KINDS:
        return ref.process(x.float(), proc, exact=True).to(F16)
    return ref.process(x, proc, exact=True)


@functools.lru_cache(maxsize=None)
def _case_probs(key, kind):
    return probs(ngram_case(*key).x, kind).double().numpy()


def case_probs(key, kind):
    """fp64 [B, γ'+1, V] of the case ngram_case(*key) under processor `kind` (cached; do not modify)."""
    return _case_probs(tuple(key), kind)


def quiet_offset(P, drafts, stoch, row_base=0, stops=(), seed=NOISE_SEED, start=OFFSET, limit=32):
    """(offset, rows): the lowest Philox offset from `start` on at which no draw that the rows' walks
    reach is close — chosen on the host, before anything runs on the device."""
    for off in range(start, start + limit):
        rows = ngram_rows(P, drafts, stoch, seed, off, row_base, stops)
        if not any(r.close for r in rows):
            return off, rows
    raise LookupError("no quiet offset")


# ---------------------------------------------------------------- the GPU grid
STEP_SHAPES = [(B, g, V, dtype) for B in (1, 5) for g in (4, 8) for V in (9, 1000, 2049, 4101) for dtype in (BF16, F32)] + \
              [(B, g, 1000, F16) for B in (1, 5) for g in (4, 8)]
ROW_BASES = (0, 1000)
FILLER_KS = (0, 3)


def step_key(B, g, V, dtype):
    return (B, g, V, dtype, re_.seed_of("ngram-philox", B, g, V))


def step_host(B, g, V, dtype, kind, row_base, stops=()):
    """(case, P, off, rows) of one cell of the one-call grid at its quiet offset."""
    key = step_key(B, g, V, dtype)
    case, P = ngram_case(*key), case_probs(key, kind)
    off, rows = quiet_offset(P, case.drafts.tolist(), KINDS[kind].stochastic, row_base, stops)
    return case, P, off, rows


# chunked windows: rows 0..30 all but certain (odds 400), rows from 31 on at odds 6; planned mismatches at
# 31, 32, inside chunk 1 and none, rotated over the cases so that every case has three of the four
CHUNK_SHAPES = [(33, 2049, BF16), (40, 2049, BF16), (33, 1000, F32), (40, 1000, F32)]
CHUNK_B = 3
CHUNK_KINDS = ("multi_t1", "greedy")


def chunk_key(g, V, dtype):
    inside = 36 if g > 36 else None
    plans = [31, 32, inside, None]
    rot = CHUNK_SHAPES.index((g, V, dtype))
    plan = tuple(plans[(rot + j) % 4] for j in range(CHUNK_B))
    return (CHUNK_B, g, V, dtype, re_.seed_of("ngram-philox-chunked", g, V), 400.0, 6.0, plan)


def chunk_host(g, V, dtype, kind, stops=()):
    key = chunk_key(g, V, dtype)
    case, P = ngram_case(*key), case_probs(key, kind)
    off, rows = quiet_offset(P, case.drafts.tolist(), KINDS[kind].stochastic, 0, stops, limit=64)
    return case, P, off, rows


# ---------------------------------------------------------------- shards and stops
SHARD_B, SHARD_ROW_BASE = 6, 1000
SHARD_KINDS = ("multi_t1", "topk20", "greedy")


def shard_host(kind):
    """(case, P, off, rows): B = 6, γ' = 8, V = 2049 bf16 at row_base 1000, run as one call and as rows
    [0, 3) + [3, 6)."""
    key = (SHARD_B, 8, 2049, BF16, re_.seed_of("ngram-philox-shards"))
    case, P = ngram_case(*key), case_probs(key, kind)
    off, rows = quiet_offset(P, case.drafts.tolist(), KINDS[kind].stochastic, SHARD_ROW_BASE)
    return case, P, off, rows


STOP_KINDS = ("greedy", "multi_t1")


def step_stop_case(kind):
    """(case, P, off, rows, b, stops): B = 5, γ' = 8, V = 2049 bf16 with the stop list [drafts[b][2],
    drafts[b][0]] of a row b whose free walk accepts at least three drafts: the first-listed stop is at
    position 2."""
    key = step_key(5, 8, 2049, BF16)
    case, P = ngram_case(*key), case_probs(key, kind)
    _, free = quiet_offset(P, case.drafts.tolist(), KINDS[kind].stochastic)
    b = next(b for b, r in enumerate(free) if r.n >= 3)
    stops = [int(case.drafts[b, 2]), int(case.drafts[b, 0])]
    off, rows = quiet_offset(P, case.drafts.tolist(), KINDS[kind].stochastic, 0, stops)
    return case, P, off, rows, b, stops


def chunk_stop_case(g, V, dtype, kind):
    """The chunked case with the stop list [drafts[b][33], drafts[b][1]] of a row b that accepts at least 34
    drafts (None where the case has no such row)."""
    case, P, off, rows = chunk_host(g, V, dtype, kind)
    b = next((b for b, r in enumerate(rows) if r.n >= 34), None)
    if b is None:
        return None
    stops = [int(case.drafts[b, 33]), int(case.drafts[b, 1])]
    case, P, off, rows = chunk_host(g, V, dtype, kind, tuple(stops))
    return case, P, off, rows, b, stops
