"""The row and verify kernels at the low end of V, on rows that are not packed slices of a bigger tensor.

Every GPU test elsewhere runs at V >= 2048 on packed [B, n, V] slices, so the bytes after a row's last
element are another valid row and "aligned row start, ragged V" only occurs where 8 | V.  Here
(tests/row_edges.py): V below, at and above one 16-byte vector (4 fp32 / 8 16-bit elements), one wave,
one fp32 stage (1024) and one span (2048); rows with -inf entries; and three layouts inside a buffer
poisoned with +inf or NaN (packed, padded to an aligned stride, shifted by one element), so an
element read from outside [0, V) shows in a max, a sum or a draw.

* sd_probs against the exact-arithmetic oracle with the kernel's tie rule, tolerances of
  test_gpu_parity.py::test_probs_rows_close_to_oracle (the share of differing 16-bit elements only
  where R * V >= 4096; below, every differing element within one ulp); masked entries exactly 0.
* sd_sample under STREAM noise: tokens equal one of the oracle variants, the generator advanced as
  the oracle's, no masked token, and sd_last_sample_path pinned from both sides of the vector
  paths' guards (16-bit V < 8 never the lean / stream kernels; padded 16-bit V >= 8 at T = 1 always).
* sd_verify under STREAM: test_gpu_parity.py's check_spec and _engine_case (bit-exact integer
  outputs and generator state) with the rows placed in the layouts.
* sd_verify under PHILOX on every path selection (lean, fused, ticket, two-launch): the per-row
  assertions of test_gpu_gamma_edges.py::check_walk against perf_walk.host_rows, row_counts, the
  path from sd_last_verify_path, and all selections' integer outputs equal row for row.  The seeds
  (row_edges.PHILOX_SEEDS) are proven on the host by tests/test_row_edges_cpu.py: no close call,
  an accepting and a rejecting row in every case — nothing here is skipped.

k_verify_lean needs V >= 8 (one whole vector inside the row: ld16_clamped's precondition); below it
launch_verify_lean declines and the fused / two-launch kernels, which guard their vector loads, run.
"""
import collections
import contextlib
import dataclasses
import math
from types import SimpleNamespace

import pytest
import torch

import perf_walk as pw
import row_edges as re_
import test_gpu_gamma_edges as ge
import test_gpu_parity as par
from oracle import specdec_ref as ref
from row_edges import BF16, DTYPES, F16, F32, LAYOUTS, V_GRID, dt_name
from test_gpu_perfmode import verify

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 4                       # rows per row-kernel call
STATS = collections.Counter()


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise, StreamNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, StreamNoise=StreamNoise)


def placer(layout, *key):
    poison = re_.poison_of(layout, *key)
    return lambda t: re_.place(t, layout, poison, DEV)


seed_of = re_.seed_of


GRID = [(V, dtype, layout) for V in V_GRID for dtype in DTYPES for layout in LAYOUTS]
GRID_IDS = [f"V{V}-{dt_name(d)}-{lay}" for V, d, lay in GRID]


# ---------------------------------------------------------------- sd_probs
def check_probs(sd, x, xd, proc, label):
    want = ref.process(x, dataclasses.replace(proc, stable_ties=True), exact=True)
    got = sd.ops.probs_rows(xd, par.spec_of(sd, proc)).cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert bool((got[torch.isinf(x) & (x < 0)] == 0).all()), label       # masked entries: exactly 0
    assert torch.equal(got > 0, want > 0), (label, (got > 0).sum(-1), (want > 0).sum(-1))
    if x.dtype == F32:
        torch.testing.assert_close(got, want, rtol=2e-6, atol=1e-12, msg=lambda m: f"{label}: {m}")
        return
    diff = got != want
    if x.numel() >= 4096:
        assert diff.float().mean().item() < 2e-3, label
    else:
        assert bool(re_.within_one_ulp(got, want)[diff].all()), (label, got[diff], want[diff])
    torch.testing.assert_close(got.float(), want.float(), rtol=8e-3, atol=1e-9, msg=lambda m: f"{label}: {m}")


@pytest.mark.parametrize("V,dtype,layout", GRID, ids=GRID_IDS)
def test_probs_rows(sd, V, dtype, layout):
    for mask in re_.MASKS:
        x = re_.logits((R, V), dtype, seed_of("probs", V, mask), mask)
        xd = placer(layout, V, dtype, mask)(x)
        for kind, proc in re_.kinds_for(dtype).items():
            check_probs(sd, x, xd, proc, f"{kind} mask={mask}")
            STATS["probs"] += 1


# ---------------------------------------------------------------- sd_sample, STREAM
def vector_sample_paths(lib):
    return (lib.SD_PATH_SAMPLE_DRAW_LEAN, lib.SD_PATH_SAMPLE_GREEDY_LEAN, lib.SD_PATH_SAMPLE_STREAM)


def check_sample(sd, x, xd, proc, kind, layout, label):
    lib = sd.lib
    g2 = torch.Generator().manual_seed(7)
    tok, _, st = sd.ops.sample_rows(xd, par.spec_of(sd, proc), sd.StreamNoise(g2))
    path = lib.last_sample_path()
    tok, st = tok.cpu(), st.cpu()
    assert not bool((st & lib.SD_ROW_ERROR_MASK).any()), (label, [hex(s) for s in st.tolist()])
    match = []
    for vlabel, pv, exact in par.oracle_variants(proc):
        g1 = torch.Generator().manual_seed(7)
        want = ref.sample(ref.process(x, pv, exact), pv, ref.TorchNoise(g1)).squeeze(-1)
        if torch.equal(tok, want):
            match.append(vlabel)
    assert match, (label, tok, want)
    STATS["sample"] += 1
    STATS["rows"] += x.shape[0]
    if match[0] != "cpu":
        STATS["non_cpu_rows"] += x.shape[0]
    # 2 R V words for a stochastic processor, none for greedy
    assert torch.equal(g2.get_state(), g1.get_state()), label
    if not proc.stochastic:
        assert torch.equal(g2.get_state(), torch.Generator().manual_seed(7).get_state())
    assert bool((x.float()[torch.arange(x.shape[0]), tok] > -math.inf).all()), (label, tok)   # never a masked token
    V = x.shape[-1]
    if x.dtype != F32 and V < 8:
        assert path not in vector_sample_paths(lib), (label, lib.PATH_NAMES.get(path))
    if x.dtype != F32 and V >= 8 and layout == "padded" and kind in ("greedy", "multi_t1"):
        want_path = lib.SD_PATH_SAMPLE_GREEDY_LEAN if kind == "greedy" else lib.SD_PATH_SAMPLE_STREAM
        assert path == want_path, (label, lib.PATH_NAMES.get(path))
    STATS[f"sample:{lib.PATH_NAMES.get(path)}"] += 1


@pytest.mark.parametrize("V,dtype,layout", GRID, ids=GRID_IDS)
def test_sample_rows_stream(sd, V, dtype, layout):
    for mask in re_.MASKS:
        x = re_.logits((R, V), dtype, seed_of("sample", V, mask), mask)
        xd = placer(layout, V, dtype, mask, "s")(x)
        for kind, proc in re_.kinds_for(dtype).items():
            check_sample(sd, x, xd, proc, kind, layout, f"{kind} mask={mask}")


@pytest.mark.parametrize("V,dtype,layout", GRID, ids=GRID_IDS)
def test_greedy_tie_lowest_index(sd, V, dtype, layout):
    """The maximum tied between element 0 and elements of the row's last (partial) vector, the last
    element among them: torch.argmax returns the lowest index."""
    x = re_.logits((R, V), dtype, seed_of("tie", V))
    vec = 4 if dtype == F32 else 8
    x[:, (V - 1) // vec * vec:] = 40.0
    x[:, 0] = 40.0
    first = (V - 1) // vec * vec
    if first > 0:
        x[R - 1, 0] = -math.inf      # one row whose lowest tied index is the last vector's first element
    xd = placer(layout, V, dtype, "tie")(x)
    gen = torch.Generator().manual_seed(7)
    tok, _, st = sd.ops.sample_rows(xd, par.spec_of(sd, re_.KINDS["greedy"]), sd.StreamNoise(gen))
    assert not bool((st.cpu() & sd.lib.SD_ROW_ERROR_MASK).any())
    assert tok.cpu().tolist() == [0] * (R - 1) + [first], tok
    assert torch.equal(gen.get_state(), torch.Generator().manual_seed(7).get_state())
    STATS["sample"] += 1


# ---------------------------------------------------------------- sd_verify, STREAM (bit-exact)
STREAM_GRID = [(V, dtype, layout) for V in V_GRID for dtype in re_.STREAM_DTYPES for layout in LAYOUTS]


@pytest.mark.parametrize("V,dtype,layout", STREAM_GRID, ids=[f"V{V}-{dt_name(d)}-{lay}" for V, d, lay in STREAM_GRID])
def test_stream_verify(sd, V, dtype, layout):
    """check_spec over B in {1, 3}, γ in {1, 4} and five processors (topk20: top_k > V at small V), and
    the ENGINE rule's _engine_case, with the rows in `layout`."""
    place = placer(layout, V, dtype, "verify")
    for B, gamma in re_.STREAM_BG:
        for kind in re_.STREAM_KINDS:
            proc = par.KINDS[kind]
            seed = re_.stream_seed(V, dtype, B, gamma, kind)
            tl, dl, ids = par.draft_case(B, gamma, V, dtype, seed, proc)
            st = par.check_spec(sd, tl, dl, ids, proc, seed, place=place)
            assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_STREAM
            STATS["verify:stream"] += 1
            STATS["nucleus_inexact"] += sum(1 for s in st if s & sd.lib.SD_ROW_NUCLEUS_INEXACT)
        par._engine_case(sd, B, gamma, V, dtype, seed_of("engine", V, B, gamma), place=place)
        STATS["verify:stream"] += 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("V", [V for V in V_GRID if V < 64])
def test_stream_verify_fp16(sd, V, layout):
    proc = par.KINDS["multi_t1"]
    seed = seed_of("spec16", V)
    tl, dl, ids = par.draft_case(3, 4, V, F16, seed, proc)
    par.check_spec(sd, tl, dl, ids, proc, seed, place=placer(layout, V, F16, "verify"))
    STATS["verify:stream"] += 1


# ---------------------------------------------------------------- sd_verify, PHILOX, every path
@contextlib.contextmanager
def selected(lib, sel):
    """test_gpu_gamma_edges.py's selections; "fused" here also turns the lean kernel off, so that a
    B = 8 call (which the lean kernel takes first) reaches k_verify_fused."""
    with contextlib.ExitStack() as st:
        if sel == "fused":
            st.enter_context(lib.option(lib.SD_OPT_LEAN_VERIFY, 0))
        st.enter_context(ge.selected(lib, sel))
        yield


def expected_path(lib, c, aligned):
    """test_gpu_gamma_edges.py's expected_path with the lean kernel's real condition on the rows: every
    row start 16-byte aligned and V >= 8 (there: V % 8 == 0, the same thing for packed rows)."""
    n_t = c.gamma + (1 if c.rule == "spec" else 0)
    if c.sel == "two-launch":
        return lib.SD_PATH_VERIFY_TWO_LAUNCH
    # the lean kernel computes the drafter rows' statistics itself when the draws' do not come along
    if (c.sel != "fused" and c.B <= ge.LEAN_MAX_B and c.gamma <= ge.LEAN_MAX_GAMMA and c.dtype in (BF16, F16)
            and aligned and c.V >= 8):
        return lib.SD_PATH_VERIFY_LEAN
    if not c.draws:                  # k_verify_fused takes the drafter statistics from the draws
        return lib.SD_PATH_VERIFY_TWO_LAUNCH
    if c.B >= 8 and n_t <= ge.FUSED_MAX_TSLOTS:
        ticket = c.sel == "ticket" or c.B >= ge.TICKET_MIN_B
        return lib.SD_PATH_VERIFY_FUSED_TICKET if ticket else lib.SD_PATH_VERIFY_FUSED
    return lib.SD_PATH_VERIFY_TWO_LAUNCH


def run_philox(sd, c, pc, layout):
    """test_gpu_gamma_edges.py's run_walk for one call, the rows placed in `layout`; also row_counts."""
    case, g, B = pc.case, c.gamma, c.B
    engine = c.rule == "engine"
    n_t = g if engine else g + 1
    place = placer(layout, c.V, c.dtype, c.rule, g)
    tl, dl, ids = place(case.tl[:, :n_t]), place(case.dl), case.ids.to(DEV)
    kw, state = {}, None
    if engine:
        generated = torch.zeros(B, ge.STEP + g + ge.GEN_LEN_PAD, dtype=torch.long)
        generated[:, ge.STEP:ge.STEP + g] = case.ids
        state = SimpleNamespace(generated0=generated, gen=generated.to(DEV),
                                fin=torch.zeros(B, dtype=torch.uint8, device=DEV),
                                acc=torch.full((B,), ge.ACC0, dtype=torch.long, device=DEV),
                                active=torch.tensor(pw.active_mask(B), dtype=torch.uint8, device=DEV))
        kw = dict(stops=pc.ends, active=state.active,
                  engine_state=dict(generated=state.gen, step=ge.STEP, finished=state.fin, accepted=state.acc))
    counts = torch.zeros(B, 2, dtype=torch.long, device=DEV)
    noise = sd.PhiloxNoise(seed=pc.noise[0], offset=pc.noise[1])
    assert noise.offset == pc.noise[1]
    rule = sd.lib.SD_RULE_ENGINE if engine else sd.lib.SD_RULE_SPEC
    with selected(sd.lib, c.sel):
        out = verify(sd, tl, dl, ids, rule, pw.WALK_PROC, noise, draws=c.draws, row_counts=counts, **kw)
    aligned = re_.rows_aligned(*[tl[:, t] for t in range(n_t)], *[dl[:, d] for d in range(g)])
    want = expected_path(sd.lib, c, aligned)
    assert out.path == want, (c.id, layout, sd.lib.PATH_NAMES.get(out.path), sd.lib.PATH_NAMES.get(want))
    if c.V < 8:
        assert out.path != sd.lib.SD_PATH_VERIFY_LEAN
    res = SimpleNamespace(**{f: getattr(out, f).cpu().tolist()
                             for f in ("n_accepted", "next_token", "row_status", "prune_drafter", "prune_target",
                                       "resample_mass")})
    res.counts = counts.cpu().tolist()
    res.path = out.path
    if engine:
        res.gen, res.fin, res.acc, res.generated0 = state.gen.cpu(), state.fin.cpu(), state.acc.cpu(), state.generated0
    return res


def integer_outputs(res, b, engine):
    out = (res.n_accepted[b], res.next_token[b], res.row_status[b], res.prune_drafter[b], res.prune_target[b],
           tuple(res.counts[b]))
    if engine:
        out += (tuple(res.gen[b].tolist()), int(res.fin[b]), int(res.acc[b]))
    return out


PHILOX_GRID = [(rule, V, g, dtype) for rule in re_.PHILOX_RULES for V in re_.PHILOX_V for g in re_.PHILOX_GAMMAS
               for dtype in re_.PHILOX_DTYPES]


@pytest.mark.parametrize("rule,V,gamma,dtype", PHILOX_GRID,
                         ids=[f"{r}-V{V}-g{g}-{dt_name(d)}" for r, V, g, d in PHILOX_GRID])
def test_philox_verify_paths(sd, rule, V, gamma, dtype):
    lib = sd.lib
    for B in (8, 16):
        pc = re_.philox_case(rule, B, gamma, V, dtype)
        runs = collections.defaultdict(list)
        for sel in (s for s, b in re_.PHILOX_SELS.items() if b == B):
            for draws in (True, False):
                for layout in re_.PHILOX_LAYOUTS:
                    c = ge.Case(sel, rule, B, gamma, V, dtype, draws)
                    res = run_philox(sd, c, pc, layout)
                    got = ge.check_walk(sd, c, pc.case, pc.ends, pc.rows, res)
                    assert got.close_rows == 0          # proven on the host (tests/test_row_edges_cpu.py)
                    for b, r in enumerate(pc.rows):     # row_counts: (accepted, accepted + the drawn token)
                        want = [r.want, r.want + (res.next_token[b] >= 0)] if r.active else [0, 0]
                        assert res.counts[b] == want, (c.id, layout, b, res.counts[b], want)
                    runs[(draws, layout)].append((f"{c.id}/{layout}", res))
                    STATS[f"verify:{lib.PATH_NAMES.get(res.path)}"] += 1
                    STATS["close"] += got.close_rows
        # the same (inputs, noise, layout, stats source) on every path selection: equal integer outputs,
        # row for row (test_gpu_lean_verify.py allows B // 64 differing rows: none here)
        for group in runs.values():
            name0, res0 = group[0]
            for name, res in group[1:]:
                for b in range(B):
                    a, o = integer_outputs(res0, b, rule == "engine"), integer_outputs(res, b, rule == "engine")
                    assert a == o, (name0, name, b, a, o)


# ---------------------------------------------------------------- sd_sample, PHILOX draws
DRAW_R, DRAW_CALLS = 4096, 4          # test_gpu_draw.py::test_draw_distribution's draw count
DRAW_PROCS = {"multi_t1": ref.Processor("multinomial", 1.0), "topk50_t08": ref.Processor("topk", 0.8, 50),
              "topk2": ref.Processor("topk", 1.0, 2)}
DRAW_GRID = [(V, dtype, layout, name) for V in (3, 8, 9, 65) for dtype in (BF16, F32) for layout in ("padded", "packed")
             for name in DRAW_PROCS]


@pytest.mark.parametrize("V,dtype,layout,name", DRAW_GRID,
                         ids=[f"V{V}-{dt_name(d)}-{lay}-{n}" for V, d, lay, n in DRAW_GRID])
def test_philox_draw_distribution(sd, V, dtype, layout, name):
    """test_gpu_draw.py::test_draw_distribution (its row, draw count, chi-square and threshold) at
    small V, the 4096 copies of the row laid out in `layout`."""
    from test_gpu_draw import chi2_check, rand_logits
    import numpy as np
    proc = DRAW_PROCS[name]
    row = rand_logits((V,), dtype, 4, 1.5)
    logits = placer(layout, V, dtype, "draw")(row.view(1, V).expand(DRAW_R, V))
    probs = ref.process(row, dataclasses.replace(proc, stable_ties=True), exact=True).double()
    noise = sd.PhiloxNoise(seed=31337)
    xs = []
    for _ in range(DRAW_CALLS):
        tok, prob, st = sd.ops.sample_rows(logits, par.spec_of(sd, proc), noise, want_prob=True)
        path = sd.lib.last_sample_path()
        assert ((st & sd.lib.SD_ROW_DONE) != 0).all()
        assert ((st & sd.lib.SD_ROW_INVALID_DIST) == 0).all()
        t = tok.cpu()
        assert torch.allclose(prob.cpu(), probs[t].float(), rtol=1e-2, atol=0), name
        xs.append(t.numpy())
    chi2_check(np.concatenate(xs), probs.numpy(), f"row-edges {name} V={V} {dt_name(dtype)} {layout}")
    if dtype != F32 and V < 8:
        assert path not in vector_sample_paths(sd.lib), sd.lib.PATH_NAMES.get(path)
    STATS[f"sample:{sd.lib.PATH_NAMES.get(path)}"] += 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_name)
@pytest.mark.parametrize("V", V_GRID)
def test_philox_draw_row_stats(sd, V, dtype, layout):
    """test_gpu_draw.py::test_draw_row_stats_reproduce_softmax: exp(y - M) / S from the draw's (M, S) is
    the row's softmax (fp64) to 2e-6 relative on the largest probabilities; masked rows included."""
    for mask in re_.MASKS:
        x = re_.logits((R, V), dtype, seed_of("stats", V, mask), mask)
        stats = torch.empty(R, 2, dtype=torch.float32, device=DEV)
        tok, prob, st = sd.ops.sample_rows(placer(layout, V, dtype, mask, "stats")(x), par.spec_of(sd, par.KINDS["multi_t1"]),
                                           sd.PhiloxNoise(seed=7), want_prob=True, row_stats_out=stats)
        path = sd.lib.last_sample_path()
        assert ((st & sd.lib.SD_ROW_ERROR_MASK) == 0).all(), (mask, st)
        xc = x.double()
        M, S = stats[:, 0].double().cpu(), stats[:, 1].double().cpu()
        p = torch.exp(xc - M[:, None]) / S[:, None]
        exact = torch.softmax(xc, dim=-1)
        top = exact >= exact.max(dim=-1, keepdim=True).values * 1e-3
        rel = ((p - exact).abs() / exact)[top]
        assert float(rel.max()) < 2e-6, (mask, float(rel.max()))
        t = tok.cpu()
        assert ((t >= 0) & (t < V)).all()
        assert bool((xc[torch.arange(R), t] > -math.inf).all()), (mask, t)        # never a masked token
        want = ref.softmax(x, True).float()
        got = prob.cpu()
        for r in range(R):
            assert got[r] == want[r, t[r]] or abs(float(got[r]) - float(want[r, t[r]])) <= 1e-2 * float(want[r, t[r]])
        if dtype != F32 and V < 8:
            assert path not in vector_sample_paths(sd.lib), sd.lib.PATH_NAMES.get(path)
        if dtype != F32 and V >= 8 and layout == "padded":
            assert path == sd.lib.SD_PATH_SAMPLE_DRAW_LEAN, sd.lib.PATH_NAMES.get(path)
        STATS[f"sample:{sd.lib.PATH_NAMES.get(path)}"] += 1


# ---------------------------------------------------------------- sd_ngram_verify, one step
NGRAM_KINDS = ("greedy", "multi_t1", "multi_t07", "topk20", "nucleus09")
NGRAM_GRID = [(V, K, dtype, layout) for V in (5, 9, 65, 2049) for K in ("0", "1", "V") for dtype in (BF16, F32)
              for layout in LAYOUTS]


@pytest.mark.parametrize("V,K,dtype,layout", NGRAM_GRID, ids=[f"V{V}-k{K}-{dt_name(d)}-{lay}" for V, K, d, lay in NGRAM_GRID])
def test_ngram_verify_step(sd, V, K, dtype, layout):
    """test_gpu_parity.py::test_ngram_verify_step_matches_oracle's construction (peaked rows, the first
    `match` drafts right) and assertions, γ' = 4, with filler_k 0, 1 and V."""
    K = {"0": 0, "1": 1, "V": V}[K]
    g, n_match = 4, 2
    for kind in NGRAM_KINDS:
        proc = par.KINDS[kind]
        seed = seed_of("ngram", V, kind)
        x = par.rand_logits((g + 1, V), torch.float32, seed, 3.0)
        hot = torch.randint(0, V, (g + 1,), generator=torch.Generator().manual_seed(seed + 1))
        x[torch.arange(g + 1), hot] += 25.0
        x = x.to(dtype)
        drafts = [int(hot[i]) if i < n_match else (int(hot[i]) + 1) % V for i in range(g)]
        stops = [3]
        variants = {}
        for exact in (False, True):
            gen = torch.Generator().manual_seed(5000 + seed)
            n, xo = ref.ngram_verify_step(x, drafts, proc, ref.TorchNoise(gen))
            variants[exact] = (n, xo, ref.stop_location(drafts[:n], stops), gen.get_state())
        gen2 = torch.Generator().manual_seed(5000 + seed)
        xd = placer(layout, V, dtype, "ngram")(x)
        out = sd.ops.ngram_verify([xd[i:i + 1] for i in range(g + 1)], torch.tensor([drafts], dtype=torch.long, device=DEV),
                                  par.spec_of(sd, proc), sd.StreamNoise(gen2),
                                  torch.tensor(stops, dtype=torch.long, device=DEV), filler_k=K)
        torch.cuda.synchronize()
        assert not int(out.row_status[0]) & sd.lib.SD_ROW_ERROR_MASK
        got = (int(out.n_accepted[0]), int(out.next_token[0]), int(out.stop_index[0]))
        # a stop among the accepted drafts returns before x is drawn: the oracle step drew x anyway
        ok = [exact for exact, (n_o, x_o, stop_o, state) in variants.items()
              if got == (n_o, -1 if stop_o >= 0 else x_o, stop_o)
              and (stop_o >= 0 or torch.equal(gen2.get_state(), state))]
        assert ok, (kind, got, variants)
        STATS["ngram"] += 1
        if K:
            p = ref.process(x, proc, True).float()
            ids = out.filler_ids[0].cpu()
            for i in range(g + 1):
                assert len(set(ids[i].tolist())) == K and 0 <= int(ids[i].min()) and int(ids[i].max()) < V
                if re_.rank_close(x[i]):       # logits an fp32 exponent cannot tell apart: values, not ranks
                    torch.testing.assert_close(p[i][ids[i]], p[i].topk(K).values, rtol=re_.RANK_CLOSE_RTOL, atol=0)
                    STATS["rank_close"] += 1
                    continue
                assert torch.equal(p[i][ids[i]], p[i].topk(K).values), (kind, i, ids[i], p[i].topk(K))
        else:
            assert out.filler_ids is None


# ---------------------------------------------------------------- processor extremes
def check_extreme_probs(sd, x, xd, name, proc, label):
    """sd_probs at a processor extreme: the kept set, then the values against the exact softmax over it."""
    T = proc.temperature
    got = sd.ops.probs_rows(xd, par.spec_of(sd, proc)).cpu()
    st_proc = dataclasses.replace(proc, stable_ties=True)
    exact = ref.process(x, st_proc, exact=True)
    assert bool((got[torch.isinf(x) & (x < 0)] == 0).all()), label
    if name in ("nucleus0", "nucleus1e-06"):
        # exactly one survivor: rank 0, the lowest index among equal maxima
        assert (got > 0).sum(-1).tolist() == [1] * x.shape[0], (label, (got > 0).sum(-1))
        assert torch.equal(got.float().argmax(-1), x.float().argmax(-1)), label
    if name == "nucleus1":
        # the cut is decided by rounding alone: an unflagged row (the search reproduced the fp32 cumsum) keeps
        # the torch-arithmetic or the exact oracle's set, a row flagged SD_ROW_NUCLEUS_INEXACT may keep
        # either or its own; in every case at most the project's mass tolerance is dropped
        cpu = ref.process(x, st_proc, exact=False)
        keep = torch.zeros(x.shape[0], 4, dtype=torch.int32, device=DEV)
        _, _, st = sd.ops.sample_rows(xd, par.spec_of(sd, proc), sd.StreamNoise(torch.Generator().manual_seed(1)),
                                      row_keep_out=keep)
        flags = (st.cpu() | keep[:, 2].cpu()).tolist()
        for r in range(x.shape[0]):
            kept = got[r] > 0
            if flags[r] & sd.lib.SD_ROW_NUCLEUS_INEXACT:
                STATS["nucleus_inexact"] += 1
                continue
            assert torch.equal(kept, cpu[r] > 0) or torch.equal(kept, exact[r] > 0), (label, r, int(kept.sum()))
        assert float(re_.dropped_mass(x, got > 0).max()) <= par.MASS_TOL, label
        want = re_.kept_softmax(x, got > 0, T)
    elif T == re_.COLD_T:
        # small probabilities underflow differently in fp32 and fp64 arithmetic: values, not supports
        want = exact
    else:
        assert torch.equal(got > 0, exact > 0), (label, (got > 0).sum(-1), (exact > 0).sum(-1))
        want = exact
    if x.dtype == F32:
        rtol = re_.COLD_RTOL_F32 if T == re_.COLD_T else 2e-6
        torch.testing.assert_close(got, want, rtol=rtol, atol=1e-12, msg=lambda m: f"{label}: {m}")
        return
    diff = got != want
    if T == re_.COLD_T:        # differences inside the absolute tolerance (underflow to 0) are not ulp-counted
        diff &= (got.float() - want.float()).abs() > 1e-9
    if x.numel() >= 4096:
        assert diff.float().mean().item() < 2e-3, label
    else:
        assert bool(re_.within_one_ulp(got, want)[diff].all()), (label, got[diff], want[diff])
    torch.testing.assert_close(got.float(), want.float(), rtol=8e-3, atol=1e-9, msg=lambda m: f"{label}: {m}")


def run_extreme(sd, x, place, name, proc, layout, label):
    xd = place(x)
    check_extreme_probs(sd, x, xd, name, proc, label)
    STATS["probs"] += 1
    check_sample(sd, x, xd, proc, name, layout, label)


EXTREME_GRID = [(V, dtype, layout) for V in re_.EXTREME_V for dtype in re_.EXTREME_DTYPES for layout in LAYOUTS]


@pytest.mark.parametrize("V,dtype,layout", EXTREME_GRID, ids=[f"V{V}-{dt_name(d)}-{lay}" for V, d, lay in EXTREME_GRID])
def test_processor_extremes_rows(sd, V, dtype, layout):
    """sd_probs (kept set and values) and sd_sample under STREAM (tokens, generator state) with top_k in
    {1, V - 1, V, V + 1, 1e6}, top_p in {0, 1e-6, 0.999, 1}, T in {0.05, 5} and topknucleus(3, 0.9, T = 0.05),
    over plain, masked and tied rows."""
    for mask in re_.EXTREME_MASKS:
        x = re_.extreme_logits(R, V, dtype, mask)
        place = placer(layout, V, dtype, mask, "x")
        for name, proc in re_.extreme_procs(V).items():
            run_extreme(sd, x, place, name, proc, layout, f"{name} mask={mask}")


@pytest.mark.parametrize("V,dtype,layout", EXTREME_GRID, ids=[f"V{V}-{dt_name(d)}-{lay}" for V, d, lay in EXTREME_GRID])
def test_processor_extremes_verify(sd, V, dtype, layout):
    """check_spec (accept count, token, prune lengths, generator state: exact against an oracle variant)
    at B = 1, γ = 4 with every extreme processor."""
    place = placer(layout, V, dtype, "xv")
    for name, proc in re_.extreme_procs(V).items():
        seed = re_.extreme_spec_seed(V, name)
        tl, dl, ids = par.draft_case(1, 4, V, dtype, seed, proc)
        st = par.check_spec(sd, tl, dl, ids, proc, seed, place=place)
        STATS["verify:stream"] += 1
        STATS["nucleus_inexact"] += sum(1 for s in st if s & sd.lib.SD_ROW_NUCLEUS_INEXACT)


BIG_PROCS = sorted(re_.extreme_procs(re_.BIG_V))


@pytest.mark.parametrize("name", BIG_PROCS)
def test_processor_extremes_big_vocab(sd, name):
    """One bf16 row batch at V = 128256 (padded rows) per extreme processor."""
    V = re_.BIG_V
    x = re_.extreme_logits(3, V, BF16, "half")
    run_extreme(sd, x, placer("padded", V, BF16, "big"), name, re_.extreme_procs(V)[name], "padded", f"{name} V={V}")


def test_summary():
    paths = {k: v for k, v in sorted(STATS.items()) if ":" in k}
    print(f"[row-edges] cases per path: {paths}; probs cases: {STATS['probs']}; n-gram steps: {STATS['ngram']}; "
          f"sample cases: {STATS['sample']} "
          f"({STATS['non_cpu_rows']} of {STATS['rows']} rows matched a non-torch-CPU oracle variant); "
          f"rows flagged SD_ROW_NUCLEUS_INEXACT: {STATS['nucleus_inexact']}; close calls: {STATS['close']}")
    assert STATS["close"] == 0
