"""The PHILOX verify kernels against the oracle where γ = 4 with two stop tokens never goes: γ = 1..32 on
every path (k_verify_lean, k_verify_fused in block-id and ticket order, k_stats + k_sample), stop
lists in all three regimes of the tails, and the sampled token's chunk.

(a) Accept walks.  tests/perf_walk.py builds inputs whose host walk (exact-arithmetic oracle, numpy
    Philox) is certain to reach the first and last draft of every Philox block of four accept
    uniforms and the last draft, and is a coin flip there; tests/test_perf_walk_cpu.py proves on the
    host, for exactly the cases listed here, that every such index is reached, that accepts and rejects
    happen at indices >= 4 and >= 8, and that no row is a close call.  The per-row assertions are
    those of tests/test_gpu_perfmode.py.  A draft index >= 4 reads Philox block i >> 2 and, from
    γ = 5 on, sits on a lane >= 1 of its wave in the fused and two-launch tails.
(b) Chunk pick.  The row's sampling chunk is a deterministic function of cdf_uniform(seed, offset,
    global row) and the chunk masses: the token's chunk must lie in perf_walk.chunk_bracket of the
    exact-oracle weights (width 2048 on every path: set_rchunks' one stage, k_verify_fused's
    kThreads * kFusedEpt, k_verify_lean's kSpan), which is one chunk unless u·Σ is within 1e-5·Σ of a
    chunk boundary (at most one such row per case, proven on the host).
(c) Stop lists of 1..300 entries: staged in LDS up to 64, re-read from global memory above, 8-bit
    stop ranks saturating at 255 (exact rank recomputed from listed position 254 on).

The path every call took is asserted from sd_last_verify_path against sd_verify's dispatch rules:
k_verify_lean takes B <= 8, γ <= 8, aligned 16-bit rows; k_verify_fused B >= 8 with at most 17 target
rows (γ <= 16 under SPEC, <= 17 under ENGINE); everything else the two launches — so at γ = 31, 32
every selection runs k_stats + k_sample (their general decide tail), which is asserted, not assumed.

Tolerances: integer outputs exact unless the host walk flags a close call (|u − p/q| <= 1e-6, at most
one row per case; none in the cases here); residual mass within 1e-5 + flip_slack; chunk within
chunk_bracket(tol = 1e-5).
"""
import contextlib
from types import SimpleNamespace
from typing import NamedTuple

import pytest
import torch

import perf_walk as pw
from oracle import specdec_ref as ref
from test_gpu_perfmode import verify

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
GAMMAS = (1, 2, 3, 5, 8, 9, 16, 31, 32)
RULES = ("spec", "engine")
# the Philox (seed, offset) of tests/test_gpu_perfmode.py's walks; a case adds its CASE_SEEDS entry to
# the offset (noise_of)
NOISE = {"spec": (0x1234_5678_9ABC, 5), "engine": (99, 1 << 33)}
LEAN_MAX_GAMMA = 8        # SD_LEAN_MAX_GAMMA (csrc/sd_verify_lean.inc)
LEAN_MAX_B = 8            # kLeanVerifyMaxB
FUSED_MAX_TSLOTS = 17     # kFastSlots: target rows the fused / poll-mode decide tails hold
TICKET_MIN_B = 64         # kTicketMinB


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise, StreamNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, StreamNoise=StreamNoise)


class Case(NamedTuple):
    sel: str                  # how the path is selected: lean | fused | ticket | default | two-launch
    rule: str
    B: int
    gamma: int
    V: int
    dtype: torch.dtype
    draws: bool               # drafter stats from real sample_rows draws (else computed in the verify)
    kind: str = "edge"        # perf_walk.edge_walk_case | long_walk_case
    row_base: int = 0
    shards: bool = False      # two calls of B / 2 rows with row_base = the shard's first row

    @property
    def id(self):
        name = str(self.dtype).split(".")[-1]
        return (f"{self.sel}-{self.rule}-B{self.B}-g{self.gamma}-V{self.V}-{name}"
                f"{'' if self.draws else '-stats-in-verify'}{'-long' if self.kind == 'long' else ''}"
                f"{f'-base{self.row_base}' if self.row_base else ''}{'-sharded' if self.shards else ''}")


def _walk_cases():
    out = []
    for rule in RULES:
        for g in GAMMAS:
            if g <= LEAN_MAX_GAMMA:
                out.append(Case("lean", rule, 8, g, 2048 if g < 5 else 4096, BF16, True))
            out.append(Case("fused", rule, 16, g, 4096, BF16, True))
            out.append(Case("ticket", rule, 16, g, 4096, BF16, True))
            out.append(Case("two-launch", rule, 16, g, 4096, BF16, True))
            out.append(Case("two-launch", rule, 16, g, 4096, BF16, False))
        out.append(Case("lean", rule, 8, 8, 4096, F16, True))
        out.append(Case("fused", rule, 8, 9, 2048, BF16, True))              # one past the lean kernel's γ
        out.append(Case("default", rule, 64, 16, 2048, BF16, True, kind="long"))
        out.append(Case("two-launch", rule, 16, 9, 6149, F32, True))         # ragged V, fp32
        out.append(Case("two-launch", rule, 16, 9, 6149, F32, False))
        out.append(Case("fused", rule, 8, 5, 50257, BF16, True))             # unaligned 16-bit rows: not lean
        out.append(Case("fused", rule, 16, 16, 4096, BF16, True, row_base=1000))
        out.append(Case("lean", rule, 16, 5, 4096, BF16, True, shards=True))
        out.append(Case("fused", rule, 16, 16, 4096, BF16, True, shards=True))
    return out


WALK_CASES = _walk_cases()

# One number per set of inputs: the seed of the inputs and the distance of the call's Philox offset
# from its rule's base.  The drafts at and after a pivot have p/q ~ 0.5 whatever the input seed, so
# which walks accept is decided by the uniforms: the lowest number was taken for which the host-side
# coverage conditions hold (tests/test_perf_walk_cpu.py checks every one of them).
# Key: (kind, rule, B, γ, V, dtype, row_base).
CASE_SEEDS = {
    ("edge", "spec", 8, 1, 2048, BF16, 0): 0,
    ("edge", "spec", 16, 1, 4096, BF16, 0): 0,
    ("edge", "spec", 8, 2, 2048, BF16, 0): 0,
    ("edge", "spec", 16, 2, 4096, BF16, 0): 0,
    ("edge", "spec", 8, 3, 2048, BF16, 0): 0,
    ("edge", "spec", 16, 3, 4096, BF16, 0): 0,
    ("edge", "spec", 8, 5, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 5, 4096, BF16, 0): 0,
    ("edge", "spec", 8, 8, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 8, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 9, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 16, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 31, 4096, BF16, 0): 0,
    ("edge", "spec", 16, 32, 4096, BF16, 0): 0,
    ("edge", "spec", 8, 8, 4096, F16, 0): 0,
    ("edge", "spec", 8, 9, 2048, BF16, 0): 13,
    ("long", "spec", 64, 16, 2048, BF16, 0): 0,
    ("edge", "spec", 16, 9, 6149, F32, 0): 0,
    ("edge", "spec", 8, 5, 50257, BF16, 0): 0,
    ("edge", "spec", 16, 16, 4096, BF16, 1000): 0,
    ("edge", "engine", 8, 1, 2048, BF16, 0): 0,
    ("edge", "engine", 16, 1, 4096, BF16, 0): 0,
    ("edge", "engine", 8, 2, 2048, BF16, 0): 0,
    ("edge", "engine", 16, 2, 4096, BF16, 0): 0,
    ("edge", "engine", 8, 3, 2048, BF16, 0): 0,
    ("edge", "engine", 16, 3, 4096, BF16, 0): 0,
    ("edge", "engine", 8, 5, 4096, BF16, 0): 0,
    ("edge", "engine", 16, 5, 4096, BF16, 0): 0,
    ("edge", "engine", 8, 8, 4096, BF16, 0): 6,
    ("edge", "engine", 16, 8, 4096, BF16, 0): 0,
    ("edge", "engine", 16, 9, 4096, BF16, 0): 11,
    ("edge", "engine", 16, 16, 4096, BF16, 0): 0,
    ("edge", "engine", 16, 31, 4096, BF16, 0): 0,
    ("edge", "engine", 16, 32, 4096, BF16, 0): 0,
    ("edge", "engine", 8, 8, 4096, F16, 0): 6,
    ("edge", "engine", 8, 9, 2048, BF16, 0): 238,
    ("long", "engine", 64, 16, 2048, BF16, 0): 7,
    ("edge", "engine", 16, 9, 6149, F32, 0): 11,
    ("edge", "engine", 8, 5, 50257, BF16, 0): 0,
    ("edge", "engine", 16, 16, 4096, BF16, 1000): 0,
}


def seed_key(c):
    return (c.kind, c.rule, c.B, c.gamma, c.V, c.dtype, c.row_base)


def noise_of(c):
    """The Philox (seed, offset) of case c's verify call(s)."""
    seed, off = NOISE[c.rule]
    return seed, off + CASE_SEEDS[seed_key(c)]


def host_side(c, n_ends=0):
    """(case, ends, late, rows) of a walk case: the cached inputs with their oracle probabilities, the
    ENGINE end tokens (stretched to n_ends entries by long_end_list) and the host's per-row results."""
    case = pw.walk_case(c.kind, c.B, c.gamma, c.V, c.dtype, CASE_SEEDS[seed_key(c)])
    seed, off = noise_of(c)
    if c.rule == "spec":
        return case, [], None, pw.host_rows(case, "spec", seed, off, (), c.row_base)
    active = pw.active_mask(c.B)
    ends, late = pw.engine_ends(case, seed, off, c.row_base, active)
    rows = pw.host_rows(case, "engine", seed, off, ends, c.row_base, active)
    if n_ends:
        ends = long_end_list(case, rows, ends, n_ends)
        rows = pw.host_rows(case, "engine", seed, off, ends, c.row_base, active)
    return case, ends, late, rows


def long_end_list(case, rows, ends, n):
    """`ends` stretched to n entries: fillers that occur in no draft first, the real end tokens last
    (listed positions n - len(ends) .. n - 1).  The fillers are the heaviest residual tokens of the
    rows the host walk rejects, so sampled tokens do land in the list."""
    drafts = set(case.ids.flatten().tolist()) | set(ends)
    tops = [(case.P[b, r.want].double() - case.Q[b, r.want].double()).topk(n).indices.tolist()
            for b, r in enumerate(rows) if r.active and r.rejected]
    fill = []
    for rank in range(n):
        for t in tops:
            if t[rank] not in drafts and len(fill) < n - len(ends):
                drafts.add(t[rank])
                fill.append(t[rank])
    assert len(fill) == n - len(ends)
    return fill + list(ends)


def expected_path(lib, c, B):
    """sd_verify's dispatch for a stochastic PHILOX call of B sequences (csrc/specdec_kernels.hip,
    include/specdec.h): the lean kernel first, then the fused one, else the two launches."""
    n_t = c.gamma + (1 if c.rule == "spec" else 0)
    if c.sel == "two-launch" or not c.draws:
        return lib.SD_PATH_VERIFY_TWO_LAUNCH
    if B <= LEAN_MAX_B and c.gamma <= LEAN_MAX_GAMMA and c.dtype in (BF16, F16) and c.V % 8 == 0:
        return lib.SD_PATH_VERIFY_LEAN
    if B >= 8 and n_t <= FUSED_MAX_TSLOTS:
        ticket = c.sel == "ticket" or B >= TICKET_MIN_B
        return lib.SD_PATH_VERIFY_FUSED_TICKET if ticket else lib.SD_PATH_VERIFY_FUSED
    return lib.SD_PATH_VERIFY_TWO_LAUNCH


@contextlib.contextmanager
def selected(lib, sel):
    opts = {"ticket": [(lib.SD_OPT_FUSED_TICKET, 1)],
            "two-launch": [(lib.SD_OPT_FUSED_VERIFY, 0), (lib.SD_OPT_LEAN_VERIFY, 0)],
            "fused-any": [(lib.SD_OPT_FUSED_VERIFY, 2), (lib.SD_OPT_LEAN_VERIFY, 0)],
            "ticket-any": [(lib.SD_OPT_FUSED_VERIFY, 2), (lib.SD_OPT_LEAN_VERIFY, 0), (lib.SD_OPT_FUSED_TICKET, 1)]}
    with contextlib.ExitStack() as st:
        for o, v in opts.get(sel, []):
            st.enter_context(lib.option(o, v))
        yield


STEP, GEN_LEN_PAD, ACC0 = 4, 4, 7


def run_walk(sd, c, case, ends):
    """The case's verify call(s) on the device; the outputs of all rows on the host."""
    g, B = c.gamma, c.B
    engine = c.rule == "engine"
    seed, off = noise_of(c)
    n_t = g if engine else g + 1
    tl, dl, ids = case.tl[:, :n_t].contiguous().to(DEV), case.dl.to(DEV), case.ids.to(DEV)
    state = None
    if engine:
        generated = torch.zeros(B, STEP + g + GEN_LEN_PAD, dtype=torch.long)
        generated[:, STEP:STEP + g] = case.ids
        state = SimpleNamespace(generated0=generated, gen=generated.to(DEV),
                                fin=torch.zeros(B, dtype=torch.uint8, device=DEV),
                                acc=torch.full((B,), ACC0, dtype=torch.long, device=DEV),
                                active=torch.tensor(pw.active_mask(B), dtype=torch.uint8, device=DEV))
    spans = [(0, B // 2), (B // 2, B)] if c.shards else [(0, B)]
    outs = []
    for lo, hi in spans:
        noise = sd.PhiloxNoise(seed=seed, offset=off)
        assert noise.offset == off           # the offset the call draws with (it takes the next one)
        kw = {}
        if engine:
            kw = dict(stops=ends, active=state.active[lo:hi],
                      engine_state=dict(generated=state.gen[lo:hi], step=STEP, finished=state.fin[lo:hi],
                                        accepted=state.acc[lo:hi]))
        rule = sd.lib.SD_RULE_ENGINE if engine else sd.lib.SD_RULE_SPEC
        with selected(sd.lib, c.sel):
            out = verify(sd, tl[lo:hi], dl[lo:hi], ids[lo:hi], rule, pw.WALK_PROC, noise, draws=c.draws,
                         row_base=c.row_base + lo, **kw)
        want = expected_path(sd.lib, c, hi - lo)
        print(f"[gamma-edges] {c.id}: rows {lo}..{hi - 1} took {sd.lib.PATH_NAMES.get(out.path)}")
        assert out.path == want, (sd.lib.PATH_NAMES.get(out.path), sd.lib.PATH_NAMES.get(want))
        outs.append(out)
    res = SimpleNamespace(**{f: torch.cat([getattr(o, f) for o in outs]).cpu().tolist()
                             for f in ("n_accepted", "next_token", "row_status", "prune_drafter", "prune_target",
                                       "resample_mass")})
    if engine:
        res.gen, res.fin, res.acc, res.generated0 = state.gen.cpu(), state.fin.cpu(), state.acc.cpu(), state.generated0
    return res


def check_chunk(lib, c, b, r, st, x, widened):
    """(b) the token's chunk against the bracket of the row's cdf_uniform over the oracle weights."""
    kind = ("p" if st & lib.SD_ROW_FALLBACK_P else "residual" if st & lib.SD_ROW_RESIDUAL
            else "bonus" if st & lib.SD_ROW_BONUS else None)
    assert kind == r.weights, (b, hex(st), r.weights)
    lo, hi = r.bracket
    widened.append(lo != hi)
    assert lo <= x // pw.CHUNK_WIDTH <= hi, (c.id, b, x, x // pw.CHUNK_WIDTH, (lo, hi))


def check_walk(sd, c, case, ends, rows, res):
    lib, g, V = sd.lib, c.gamma, c.V
    n, x, st, mass = res.n_accepted, res.next_token, res.row_status, res.resample_mass
    close_rows, widened = 0, []
    for b, r in enumerate(rows):
        assert not st[b] & lib.SD_ROW_ERROR_MASK, (b, hex(st[b]))
        if not r.active:             # ENGINE rows that are off: no decision, no token, state as it was
            assert not st[b] & lib.SD_ROW_DONE and n[b] == 0 and x[b] == -1, (b, hex(st[b]), n[b], x[b])
            assert torch.equal(res.gen[b], res.generated0[b]) and int(res.fin[b]) == 0 and int(res.acc[b]) == ACC0
            continue
        if n[b] != r.want:
            assert r.close, (c.id, b, n[b], r.want)
            close_rows += 1
            continue
        assert st[b] & lib.SD_ROW_DONE
        slack = 0.0
        if r.rejected:
            slack = pw.flip_slack(case.tl[b, r.want], c.dtype) + pw.flip_slack(case.dl[b, r.want], c.dtype)
        if c.rule == "spec":
            kd, kt = res.prune_drafter[b], res.prune_target[b]
            if r.want == g:
                assert st[b] & lib.SD_ROW_BONUS and kd == 0 and kt == 0
            else:
                assert st[b] & lib.SD_ROW_RESIDUAL and kd == g - r.want and kt == g - r.want + 1
                # the residual token has positive residual weight
                assert float(case.P[b, r.want, x[b]]) > float(case.Q[b, r.want, x[b]]), (b, x[b])
                assert abs(mass[b] - r.res_mass) <= pw.MASS_TOL + slack, (b, mass[b], r.res_mass, slack)
            assert 0 <= x[b] < V
            check_chunk(lib, c, b, r, st[b], x[b], widened)
            continue
        assert int(res.acc[b]) == ACC0 + r.want
        expect = res.generated0[b].clone()          # engine/infer_engine.py:326, :333-336
        if r.rejected:
            assert st[b] & (lib.SD_ROW_RESIDUAL | lib.SD_ROW_FALLBACK_P)
            assert 0 <= x[b] < V
            expect[STEP + r.want] = x[b]
            res_w = (case.P[b, r.want].double() - case.Q[b, r.want].double()).clamp(min=0)
            assert abs(mass[b] - r.res_mass) <= pw.MASS_TOL + slack, (b, mass[b], r.res_mass, slack)
            assert float(res_w[x[b]]) > 0
            assert bool(res.fin[b]) == (x[b] in ends)
            check_chunk(lib, c, b, r, st[b], x[b], widened)
        else:
            assert x[b] == -1
            assert bool(res.fin[b]) == r.finished
            assert bool(st[b] & lib.SD_ROW_FINISHED) == r.finished
        if r.want < g:
            expect[STEP + r.want + 1: STEP + g] = 0
        assert torch.equal(res.gen[b], expect), (b, res.gen[b], expect)
    assert close_rows <= 1
    assert sum(widened) <= 1
    return SimpleNamespace(close_rows=close_rows, widened=sum(widened), picked=len(widened))


@pytest.mark.parametrize("c", WALK_CASES, ids=[c.id for c in WALK_CASES])
def test_gamma_walk_and_chunk_pick(sd, c):
    """(a) + (b) of the module docstring for one case; sharded cases draw with the global row's
    uniforms (row_base = the shard's first row), row_base = 1000 with rows 1000..1015's."""
    case, ends, late, rows = host_side(c)
    res = run_walk(sd, c, case, ends)
    got = check_walk(sd, c, case, ends, rows, res)
    if late is not None:          # `finished` set from a draft at index >= 4
        lb, li = late
        assert li >= 4 and res.n_accepted[lb] == li + 1 and bool(res.fin[lb]) and res.next_token[lb] == -1
    print(f"[gamma-edges] {c.id}: {got.picked} chunk picks, {got.widened} widened, {got.close_rows} close")


# ---------------------------------------------------------------- (c) long stop lists
STOP_B, STOP_G, STOP_V = 8, 8, 4096
FIRST_DRAFT, SECOND_DRAFT = 5, 2      # row 0's drafts the two listed stop tokens are
# (list length, listed position of the first-listed hit, of the second hit or None): the first hit
# at rank 0, 63, 64, 253, 254, 255, 299 as the list's last entry, and again with a second hit (earlier
# in the draft, later in the list) behind it — in LDS, in global memory, and with saturated ranks
STOP_LISTS = [(1, 0, None), (64, 63, None), (65, 64, None), (254, 253, None), (255, 254, None), (256, 255, None),
              (300, 299, None), (64, 0, 63), (65, 63, 64), (254, 64, 253), (255, 253, 254), (256, 254, 255),
              (300, 255, 299), (300, 254, 256)]
GREEDY = ref.Processor("greedy")
# selection, processor, drafter stats from draws, the path sd_verify's dispatch takes
STOP_PATHS = [("lean", GREEDY, True, "SD_PATH_VERIFY_LEAN"),
              # a greedy SPEC target draws nothing: k_verify_fused is for stochastic rows, so these two
              # run k_stats' decide tail with (poll mode) and without the draws' stats
              ("fused-any", GREEDY, True, "SD_PATH_VERIFY_TWO_LAUNCH"),
              ("two-launch", GREEDY, False, "SD_PATH_VERIFY_TWO_LAUNCH"),
              # the fused kernel itself: a stochastic processor with drafter == target (p == q, every
              # draft accepted whatever the uniforms), so the stop outputs stay deterministic
              ("fused-any", pw.WALK_PROC, True, "SD_PATH_VERIFY_FUSED"),
              ("ticket-any", pw.WALK_PROC, True, "SD_PATH_VERIFY_FUSED_TICKET")]


def stop_inputs():
    g = torch.Generator().manual_seed(76)
    tl = (torch.randn(STOP_B, STOP_G + 1, STOP_V, generator=g) * 3).to(BF16)
    dl = tl[:, :STOP_G].clone()
    return tl, dl, dl.float().argmax(-1)


def stop_list(ids, n, first, second):
    drafts = set(ids.flatten().tolist())
    stops = [t for t in range(STOP_V) if t not in drafts][:n]      # ids that occur in no draft
    stops[first] = int(ids[0, FIRST_DRAFT])
    if second is not None:
        assert second > first
        stops[second] = int(ids[0, SECOND_DRAFT])
    return stops


@pytest.mark.parametrize("n,first,second", STOP_LISTS)
def test_long_stop_lists_stream(sd, n, first, second):
    """STREAM (the parity suite's check_spec: every integer output equals the oracle's)."""
    from test_gpu_parity import check_spec
    tl, dl, ids = stop_inputs()
    stops = stop_list(ids, n, first, second)
    assert ref.stop_location(ids[0].tolist(), stops) == FIRST_DRAFT
    st = check_spec(sd, tl, dl, ids, GREEDY, 76, stops=stops)
    assert st[0] & sd.lib.SD_ROW_STOP_IN_DRAFTS


@pytest.mark.parametrize("sel,proc,draws,path", STOP_PATHS,
                         ids=[f"{s}-{p.kind}-{'draws' if d else 'stats-in-verify'}" for s, p, d, _ in STOP_PATHS])
@pytest.mark.parametrize("n,first,second", STOP_LISTS)
def test_long_stop_lists_philox(sd, n, first, second, sel, proc, draws, path):
    """SPEC with drafter == target: every draft is accepted, and the return is at the first-LISTED stop
    token that occurs (ref.stop_location) — for hits listed past the LDS-staged 64 and past the 8-bit
    rank's 254."""
    tl, dl, ids = stop_inputs()
    stops = stop_list(ids, n, first, second)
    with selected(sd.lib, sel):
        out = verify(sd, tl.to(DEV), dl.to(DEV), ids.to(DEV), sd.lib.SD_RULE_SPEC, proc, sd.PhiloxNoise(seed=5),
                     stops=stops, draws=draws)
    print(f"[gamma-edges] stops n={n} {sel}/{proc.kind}: took {sd.lib.PATH_NAMES.get(out.path)}")
    assert out.path == getattr(sd.lib, path), sd.lib.PATH_NAMES.get(out.path)
    si, n_acc, st, x = (getattr(out, f).cpu().tolist() for f in ("stop_index", "n_accepted", "row_status", "next_token"))
    for b in range(STOP_B):
        want = ref.stop_location(ids[b].tolist(), stops)
        assert si[b] == want and n_acc[b] == STOP_G, (b, si[b], want, n_acc[b])
        assert not st[b] & sd.lib.SD_ROW_ERROR_MASK
        if want >= 0:
            assert st[b] & sd.lib.SD_ROW_STOP_IN_DRAFTS and x[b] == -1
        else:
            assert st[b] & sd.lib.SD_ROW_BONUS and 0 <= x[b] < STOP_V
    assert si[0] == FIRST_DRAFT


END_CASES = [Case("lean", "engine", 8, 8, 4096, BF16, True), Case("fused", "engine", 16, 8, 4096, BF16, True),
             Case("ticket", "engine", 16, 8, 4096, BF16, True), Case("two-launch", "engine", 16, 8, 4096, BF16, True),
             Case("two-launch", "engine", 16, 8, 4096, BF16, False)]


@pytest.mark.parametrize("n_ends", [65, 300])
@pytest.mark.parametrize("c", END_CASES, ids=[c.id for c in END_CASES])
def test_long_end_lists_engine(sd, c, n_ends):
    """ENGINE with 65 and 300 end tokens (the real ones listed last, past the LDS-staged 64): n_accepted,
    `finished` and the state equal host_walk_engine's, a sampled token that is listed finishes its row."""
    case, ends, late, rows = host_side(c, n_ends)
    assert len(ends) == n_ends and len(set(ends)) == n_ends
    res = run_walk(sd, c, case, ends)
    check_walk(sd, c, case, ends, rows, res)
    lb, li = late
    assert res.n_accepted[lb] == li + 1 and bool(res.fin[lb])
    assert any(r.active and r.finished for r in rows)
