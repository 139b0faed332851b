"""Host model of a PHILOX verify window of more than M = 32 drafts (ops.verify with γ > SD_MAX_GAMMA),
stated for the whole window at once: it does not import specdec_amd.chunked and combines nothing.

A window called with host offset `off` runs as ceil(γ / M) chunks of at most M drafts and chunk k
draws with offset off + k (every chunk is launched, so the call consumes ceil(γ / M) offsets):
  * the accept uniform of draft i of global row rb is accept_uniform(seed, off + i // M, rb, i % M);
  * SPEC (sampling/speculative_decoding.py:139-171): n is the first rejected draft of the whole
    window, else γ; the deciding chunk is k* = n // M when rejected, else (γ - 1) // M; the token is
    drawn from the residual of slot n, or the bonus row γ, on cdf_uniform(seed, off + k*, rb).  With
    a stop list the stop listed first among ids[:n] wins at its first position: no token, status
    DONE | STOP_IN_DRAFTS, prune lengths 0;
  * ENGINE (engine/infer_engine.py:297-336): the walk ends at the first reject or the first
    accepted end token; a reject at draft n draws from slot n on cdf_uniform(seed, off + n // M, rb).

Inputs are perf_walk's cached cases: the "long" kind as it is, and an "edge" kind whose pivot cycle
(window_cycle) steers rows to the drafts around the chunk edges first.  The cases the GPU file runs,
with their pinned Philox offsets, are listed here (CASES, OFFSETS); tests/test_window_walk_cpu.py
proves what they cover.  No GPU and no library import.
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

import perf_walk as pw
import philox_ref as ph
from oracle import specdec_ref as ref

M = 32                       # SD_MAX_GAMMA (tests/test_window_walk_cpu.py asserts it)
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DONE, STOP_IN_DRAFTS, FINISHED, RESIDUAL, BONUS, FALLBACK_P = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
# the rules' Philox seeds and offset bases of tests/test_gpu_gamma_edges.py
NOISE = {"spec": (0x1234_5678_9ABC, 5), "engine": (99, 1 << 33)}


def n_chunks(gamma):
    return -(-gamma // M)


def window_pivots(gamma):
    """perf_walk.pivots plus the drafts around the chunk edges: 31, 32, 33, and 63, 64 from γ = 65."""
    return pw.pivots(gamma, extra=(31, 32, 33) + ((63, 64) if gamma >= 65 else ()))


def window_cycle(gamma, B=16):
    """window_pivots in the order the rows take them: the last draft and the chunk edges first, so
    that a batch of 16 holds two rows of each (and ENGINE's inactive rows 3, 8, 13 take none away).
    B = 8 (γ >= 34): ENGINE's seven active rows must each carry one of the seven conditions that need
    a row of their own (window_walk.coverage), so six of them pivot at or after draft 31 — the last
    draft twice, 31, 32 twice, 33 — one pivots at draft 3, and the inactive row 3 takes pivot 0."""
    piv = window_pivots(gamma)
    if B == 8:
        assert gamma >= 34
        return (gamma - 1, 31, 32, 0, 33, gamma - 1, 32, 3)
    late = [gamma - 1] + [k for k in piv if k >= 31 and k != gamma - 1]
    return tuple(late + [k for k in piv if k < 31])


def accept_uniform(seed, off, rb, i):
    """Draft i of a window called at offset `off`: chunk i // M draws with offset off + i // M."""
    return ph.accept_uniform(seed, off + i // M, rb, i % M)


def inverse_cdf(weights, u):
    """The host's inverse-CDF token over fp64 weights: the first index whose running total exceeds
    u·Σ (the last positive one when none does)."""
    w = np.asarray(weights, dtype=np.float64)
    run = np.cumsum(w)
    hit = np.nonzero((run > u * run[-1]) & (w > 0))[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])


def window_rows(case, rule, seed, off, stops=(), row_base=0, active=None):
    """What the one-window rule says of every row of `case` for ops.verify with PhiloxNoise(seed, off):
    perf_walk.host_rows' fields (.active .want .close .rejected .finished .cmps .slot .weights .bracket
    .res_mass) plus
      .chunk       k*, the chunk whose cdf uniform draws the token (None: no token)
      .token       the host's inverse-CDF token on that uniform (-1: none)
      .stop_index  (SPEC) the stop's position among the accepted drafts, -1 for none
      .status      the row's status bits; .prune_drafter .prune_target
    `stops`: SPEC's stop tokens / ENGINE's end tokens."""
    g, ids, P, Q = case.gamma, case.ids, case.P, case.Q
    rows = []
    for b in range(case.B):
        r = SimpleNamespace(active=active is None or bool(active[b]), want=0, close=False, rejected=False,
                            finished=False, cmps=[], slot=None, weights=None, bracket=None, res_mass=None,
                            chunk=None, token=-1, stop_index=-1, status=0, prune_drafter=0, prune_target=0)
        rows.append(r)
        if not r.active:
            continue
        p = [float(P[b, i, ids[b, i]]) for i in range(g)]
        q = [float(Q[b, i, ids[b, i]]) for i in range(g)]
        rb = row_base + b
        if rule == "spec":
            r.want, r.close = pw.host_walk_spec(p, q, seed, off, rb, g, uniform=accept_uniform)
            r.rejected = r.want < g
            reached = min(r.want, g - 1)
            ratio = [p[i] / q[i] for i in range(g)]
            r.stop_index = ref.stop_location(ids[b, :r.want].tolist(), stops)
        else:
            r.want, r.rejected, r.finished, r.close = pw.host_walk_engine(p, q, ids[b], stops, seed, off, rb, g,
                                                                            uniform=accept_uniform)
            reached = r.want if r.rejected else r.want - 1
            ratio = [min(1.0, p[i] / q[i]) for i in range(g)]
        r.cmps = [(i, ratio[i], i < r.want) for i in range(reached + 1)]
        r.status = DONE
        if r.stop_index >= 0:
            r.status |= STOP_IN_DRAFTS
            continue
        w = None
        if r.rejected:
            w = (P[b, r.want].double() - Q[b, r.want].double()).clamp(min=0)
            r.slot, r.weights, r.res_mass, r.chunk = r.want, "residual", float(w.sum()), r.want // M
            if rule == "engine" and r.res_mass <= 1e-12:      # engine/infer_engine.py:319-321
                w, r.weights = P[b, r.want].double(), "p"
            r.status |= FALLBACK_P if r.weights == "p" else RESIDUAL
            if rule == "spec":
                r.prune_drafter, r.prune_target = g - r.want, g - r.want + 1
        elif rule == "spec":
            w = P[b, g].double()
            r.slot, r.weights, r.chunk = g, "bonus", (g - 1) // M
            r.status |= BONUS
        if w is not None:
            u = ph.cdf_uniform(seed, off + r.chunk, rb)
            r.bracket = pw.chunk_bracket(w.numpy(), u)
            r.token = inverse_cdf(w.numpy(), u)
            if rule == "engine" and r.token in stops:
                r.finished = True
        if r.finished:
            r.status |= FINISHED
    return rows


def engine_expect(case, rows, generated0, step, acc0):
    """(generated, finished, accepted) after an ENGINE window on the host's tokens: check_walk's
    `expect` construction (engine/infer_engine.py:326, :333-336); inactive rows untouched."""
    g = case.gamma
    gen = generated0.clone()
    fin = torch.zeros(case.B, dtype=torch.uint8)
    acc = torch.full((case.B,), acc0, dtype=torch.long)
    for b, r in enumerate(rows):
        if not r.active:
            continue
        acc[b] += r.want
        if r.rejected:
            gen[b, step + r.want] = r.token
        if r.want < g:
            gen[b, step + r.want + 1: step + g] = 0
        fin[b] = int(r.finished)
    return gen, fin, acc


# ---------------------------------------------------------------- the GPU grid and its pinned offsets
class Case(NamedTuple):
    rule: str
    kind: str                 # "edge" (window_cycle pivots) | "long"
    B: int
    gamma: int
    V: int
    dtype: torch.dtype
    draws: bool               # drafter stats from real sd_sample draws (else computed in the verify)
    row_base: int = 0

    @property
    def id(self):
        name = str(self.dtype).split(".")[-1]
        return (f"{self.rule}-{self.kind}-B{self.B}-g{self.gamma}-V{self.V}-{name}"
                f"{'' if self.draws else '-stats-in-verify'}{f'-base{self.row_base}' if self.row_base else ''}")

    @property
    def key(self):            # what the inputs and the walk depend on (not `draws`)
        return (self.rule, self.kind, self.B, self.gamma, self.V, self.dtype, self.row_base)


def _cases():
    out = []
    for rule in ("spec", "engine"):
        out.append(Case(rule, "edge", 16, 33, 2049, F16, False))
        for kind in ("edge", "long"):
            out.append(Case(rule, kind, 16, 40, 2048, BF16, True))
            out.append(Case(rule, kind, 16, 40, 2048, BF16, False))
            out.append(Case(rule, kind, 16, 70, 1000, F32, False))
        out.append(Case(rule, "edge", 16, 40, 2048, BF16, True, 1000))
        out.append(Case(rule, "edge", 16, 40, 2048, BF16, False, 1000))
        out.append(Case(rule, "edge", 16, 64, 2048, BF16, True))
        out.append(Case(rule, "edge", 8, 40, 4101, BF16, True, 7))
    out.append(Case("spec", "long", 1, 40, 4096, BF16, True))
    return out


CASES = _cases()
INPUT_SEED = 5
# Distance of the call's Philox offset from its rule's base (NOISE): the lowest for which the case's
# coverage conditions hold (find_offset; tests/test_window_walk_cpu.py re-proves every entry).
OFFSETS = {
    ("spec", "edge", 16, 33, 2049, F16, 0): 0,
    ("spec", "edge", 16, 40, 2048, BF16, 0): 4,
    ("spec", "edge", 16, 70, 1000, F32, 0): 0,
    ("spec", "long", 16, 40, 2048, BF16, 0): 1,
    ("spec", "long", 16, 70, 1000, F32, 0): 0,
    ("spec", "edge", 16, 40, 2048, BF16, 1000): 0,
    ("spec", "edge", 16, 64, 2048, BF16, 0): 4,
    ("spec", "edge", 8, 40, 4101, BF16, 7): 2,
    ("spec", "long", 1, 40, 4096, BF16, 0): 1,
    ("engine", "edge", 16, 33, 2049, F16, 0): 1,
    ("engine", "edge", 16, 40, 2048, BF16, 0): 5,
    ("engine", "edge", 16, 70, 1000, F32, 0): 2,
    ("engine", "long", 16, 40, 2048, BF16, 0): 93,
    ("engine", "long", 16, 70, 1000, F32, 0): 32,
    ("engine", "edge", 16, 40, 2048, BF16, 1000): 11,
    ("engine", "edge", 16, 64, 2048, BF16, 0): 8,
    ("engine", "edge", 8, 40, 4101, BF16, 7): 9,
}


def case_inputs(c):
    piv = window_cycle(c.gamma, c.B) if c.kind == "edge" else None
    return pw.walk_case(c.kind, c.B, c.gamma, c.V, c.dtype, INPUT_SEED, piv)


def window_ends(case, seed, off, row_base, active):
    """ENGINE end tokens chosen from the free walk (no end tokens): draft 31 of a row that accepts it
    (the row then finishes on the last draft of chunk 0) and a draft of chunk 1 that another row
    accepts.  Returns (ends, (row, 31) or None, (row, index >= 32) or None)."""
    free = window_rows(case, "engine", seed, off, (), row_base, active)
    at31 = next(((b, 31) for b, r in enumerate(free) if r.active and r.want >= M), None)
    later = next(((b, min(r.want - 1, 35)) for b, r in enumerate(free)
                  if r.active and r.want > M and (at31 is None or b != at31[0])), None)
    ends = [int(case.ids[x[0], x[1]]) for x in (later, at31) if x is not None]
    return ends, at31, later


@functools.lru_cache(maxsize=None)
def _host(key, delta):
    rule, kind, B, gamma, V, dtype, row_base = key
    c = Case(rule, kind, B, gamma, V, dtype, True, row_base)
    case = case_inputs(c)
    seed, off = NOISE[rule]
    off += delta
    if rule == "spec":
        return SimpleNamespace(case=case, ends=[], at31=None, later=None, seed=seed, off=off, active=None,
                               rows=window_rows(case, "spec", seed, off, (), row_base))
    active = pw.active_mask(B)
    ends, at31, later = window_ends(case, seed, off, row_base, active)
    rows = window_rows(case, "engine", seed, off, ends, row_base, active)
    return SimpleNamespace(case=case, ends=ends, at31=at31, later=later, seed=seed, off=off, active=active, rows=rows)


def host_side(c, delta=None):
    """The cached host side of case c: .case .ends .at31 .later .seed .off .active .rows."""
    return _host(c.key, OFFSETS[c.key] if delta is None else delta)


def coverage(c, h):
    """What is wrong with case c at host side h as a test input (empty: nothing).

    Every case: no close call, at most one widened chunk bracket.  Edge cases, B = 16 and B = 8: a
    reject inside chunk 0 (before draft 31), at draft 31, at draft 32, inside a later chunk (γ = 33:
    chunk 1 is draft 32 alone), and the whole window accepted; ENGINE also an end token accepted at
    draft 31, one accepted in chunk 1 and an inactive row.  Long cases at B = 16 (random walks cannot be
    steered to one draft): a row ending in chunk 0, one ending in a later chunk and one accepting the
    whole window — rejects at exactly drafts 31 and 32 are carried by the edge kinds only.  The B = 1
    case is one row, which rejects in chunk 1."""
    g, rows = c.gamma, [r for r in h.rows if r.active]
    bad = []
    if any(r.close for r in rows):
        bad.append("close rows")
    if sum(r.bracket is not None and r.bracket[0] != r.bracket[1] for r in rows) > 1:
        bad.append("more than one widened bracket")
    rej = [r.want for r in rows if r.rejected]
    full = any(r.want == g and not r.rejected and not r.finished for r in rows)
    if c.B == 1:
        return bad + ([] if rej and rej[0] >= M else ["the row does not reject in chunk 1"])
    if c.kind == "long":
        ok = any(n < M for n in rej) and any(n >= M for n in rej) and full
        return bad + ([] if ok else [f"long mix: rejects {rej}, full {full}"])
    need = {"reject in chunk 0": any(n < 31 for n in rej), "reject at 31": 31 in rej, "reject at 32": 32 in rej,
            "reject in a later chunk": any(n > M or (g == M + 1 and n == M) for n in rej), "full accept": full}
    if c.rule == "engine":
        need["end token at 31"] = h.at31 is not None and h.rows[h.at31[0]].finished and h.rows[h.at31[0]].want == M
        need["end token in chunk 1"] = (h.later is not None and h.rows[h.later[0]].finished
                                        and h.rows[h.later[0]].want == h.later[1] + 1 > M)
        need["inactive row"] = any(not r.active for r in h.rows)
    return bad + [k for k, v in need.items() if not v]


def find_offset(c, limit=4000):
    for delta in range(limit):
        if not coverage(c, host_side(c, delta)):
            return delta
    raise LookupError(c.id)


# ---------------------------------------------------------------- stops across chunks (SPEC)
STOP_FIRST, STOP_SECOND = 35, 2       # the drafts of one row that the first- and second-listed stops are


def stop_case(greedy):
    """(case, seed, off, row, stops): the γ = 40 bf16 edge case with the stop list [ids[b, 35], ids[b, 2]]
    of a row b whose walk accepts at least 36 drafts.  greedy: drafter == target rows and argmax drafts
    (every draft accepted under a greedy target, whatever the uniforms)."""
    c = Case("spec", "edge", 16, 40, 2048, BF16, True)
    h = host_side(c)
    case = h.case
    if greedy:
        ids = case.tl[:, :c.gamma].float().argmax(-1)
        case = SimpleNamespace(tl=case.tl, dl=case.tl[:, :c.gamma].clone(), ids=ids, P=None, Q=None, B=c.B,
                               gamma=c.gamma, V=c.V, dtype=c.dtype)
        b = next(b for b in range(c.B) if _stop_row_ok(ids[b]))
    else:
        b = next(b for b, r in enumerate(h.rows) if r.want >= 36 and _stop_row_ok(case.ids[b]))
    stops = [int(case.ids[b, STOP_FIRST]), int(case.ids[b, STOP_SECOND])]
    return case, h.seed, h.off, b, stops


def _stop_row_ok(ids_b):
    """The first-listed stop occurs in chunk 1 only, the second-listed one in chunk 0."""
    t = ids_b.tolist()
    return t.index(t[STOP_FIRST]) == STOP_FIRST and t[STOP_SECOND] != t[STOP_FIRST]
