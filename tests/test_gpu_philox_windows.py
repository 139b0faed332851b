"""PHILOX verify windows of more than SD_MAX_GAMMA = 32 drafts (specdec_amd/chunked.py on batches)
against the one-window host model of tests/window_walk.py.

Under Philox every chunk of a window runs on all rows at once and takes the next Philox offset, and the
chunks' outputs are combined on the device per row: rows of one call end in different chunks.  Each
case here calls ops.verify once and asserts every row against the model, which states the window's
result directly (accept uniform of draft i from offset off + i // 32, the token from the deciding
chunk's cdf uniform) and knows nothing of chunks' outputs:

* every assertion of test_gpu_gamma_edges.check_walk with g the window's γ: n, status bits, prune
  lengths against the whole γ, positive residual weight at the token, resample_mass within
  1e-5 + flip_slack, the token's sampling chunk inside chunk_bracket of the deciding chunk's cdf uniform,
  ENGINE's generated / finished / accepted with the tail past the last accepted draft zeroed, inactive
  rows untouched; no close row (the pinned offsets have none: tests/test_window_walk_cpu.py);
* row_counts added once ([n, n + (token >= 0)], inactive rows [0, 0]), status_or 0, words_used 0, and
  the noise's offset moved by ceil(γ / 32);
* two row shards with row_base equal one call; the two-launch selection equals the default one;
* SPEC stop lists whose first-listed stop occurs in chunk 1 only and whose second-listed one occurs in
  chunk 0: the return is at the first-listed stop's position (35), greedy and multinomial.

Graph safety is not tested: verify_chunked reads engine_state["step"] on the host (an int), so a
window call is not a capturable sequence of launches by construction, and no test works round that.
"""
from types import SimpleNamespace

import pytest
import torch

import perf_walk as pw
import test_gpu_gamma_edges as ge
import window_walk as ww
from oracle import specdec_ref as ref
from test_gpu_gamma_edges import ACC0, GEN_LEN_PAD, STEP
from test_gpu_perfmode import verify

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_FIELDS = ("n_accepted", "next_token", "row_status", "prune_drafter", "prune_target", "stop_index")


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise)


def run_window(sd, c, case, seed, off, ends=(), spans=None, sel="default", proc=pw.WALK_PROC, draws=None):
    """The window's verify call (one per row span, row_base = the span's first row) on the device; every
    row's outputs on the host."""
    g, B = c.gamma, c.B
    engine = c.rule == "engine"
    n_t = g if engine else g + 1
    tl, dl, ids = case.tl[:, :n_t].contiguous().to(DEV), case.dl.to(DEV), case.ids.to(DEV)
    counts = torch.zeros(B, 2, dtype=torch.long, device=DEV)
    status_or = torch.zeros(1, dtype=torch.int32, device=DEV)
    state = None
    if engine:
        generated = torch.zeros(B, STEP + g + GEN_LEN_PAD, dtype=torch.long)
        generated[:, STEP:STEP + g] = case.ids
        state = SimpleNamespace(generated0=generated, gen=generated.to(DEV),
                                fin=torch.zeros(B, dtype=torch.uint8, device=DEV),
                                acc=torch.full((B,), ACC0, dtype=torch.long, device=DEV),
                                active=torch.tensor(pw.active_mask(B), dtype=torch.uint8, device=DEV))
    outs, words, paths = [], 0, []
    for lo, hi in spans or [(0, B)]:
        noise = sd.PhiloxNoise(seed=seed, offset=off)
        kw = dict(stops=ends)
        if engine:
            kw.update(active=state.active[lo:hi],
                      engine_state=dict(generated=state.gen[lo:hi], step=STEP, finished=state.fin[lo:hi],
                                        accepted=state.acc[lo:hi]))
        rule = sd.lib.SD_RULE_ENGINE if engine else sd.lib.SD_RULE_SPEC
        with ge.selected(sd.lib, sel):
            out = verify(sd, tl[lo:hi], dl[lo:hi], ids[lo:hi], rule, proc, noise,
                         draws=c.draws if draws is None else draws, row_base=c.row_base + lo,
                         status_or=status_or, row_counts=counts[lo:hi], **kw)
        assert noise.offset == off + ww.n_chunks(g), (noise.offset, off)      # one offset per chunk
        words += int(out.words_used)
        paths.append(sd.lib.PATH_NAMES.get(out.path))
        outs.append(out)
    res = SimpleNamespace(**{f: torch.cat([getattr(o, f) for o in outs]).cpu().tolist()
                             for f in INT_FIELDS + ("resample_mass",)})
    res.counts, res.status_or, res.words, res.paths = counts.cpu().tolist(), int(status_or), words, paths
    if engine:
        res.gen, res.fin, res.acc, res.generated0 = state.gen.cpu(), state.fin.cpu(), state.acc.cpu(), state.generated0
    return res


def check_window(sd, c, h, res):
    got = ge.check_walk(sd, c, h.case, h.ends, h.rows, res)
    assert got.close_rows == 0 and got.widened <= 1
    for b, r in enumerate(h.rows):
        n, x = res.n_accepted[b], res.next_token[b]
        assert res.counts[b] == ([n, n + (x >= 0)] if r.active else [0, 0]), (b, res.counts[b], n, x)
        assert res.stop_index[b] == -1
        if r.active and r.rejected and c.rule == "engine":
            assert bool(res.row_status[b] & sd.lib.SD_ROW_FINISHED) == (x in h.ends), (b, x)
    assert res.status_or == 0 and res.words == 0
    return got


@pytest.mark.parametrize("c", ww.CASES, ids=[c.id for c in ww.CASES])
def test_window_against_host_model(sd, c):
    h = ww.host_side(c)
    res = run_window(sd, c, h.case, h.seed, h.off, h.ends)
    got = check_window(sd, c, h, res)
    for late in (h.at31, h.later):          # `finished` set from draft 31 and from a draft of chunk 1
        if late is not None:
            lb, li = late
            assert res.n_accepted[lb] == li + 1 and bool(res.fin[lb]) and res.next_token[lb] == -1
    print(f"[windows] {c.id}: last chunk took {res.paths[-1]}; {got.picked} chunk picks, {got.widened} widened, "
          f"{got.close_rows} close; n = {res.n_accepted}")


SPLIT = [ww.Case(rule, "edge", 16, 40, 2048, ww.BF16, True) for rule in ("spec", "engine")]


def ints_of(res, engine):
    out = {f: getattr(res, f) for f in INT_FIELDS}
    out["counts"] = res.counts
    if engine:
        out.update(gen=res.gen.tolist(), fin=res.fin.tolist(), acc=res.acc.tolist())
    return out


@pytest.mark.parametrize("c", SPLIT, ids=[c.id for c in SPLIT])
def test_window_row_shards_equal_one_call(sd, c):
    """Rows [0, 8) and [8, 16) with row_base = the shard's first row: the one call's integer outputs."""
    h = ww.host_side(c)
    one = run_window(sd, c, h.case, h.seed, h.off, h.ends)
    two = run_window(sd, c, h.case, h.seed, h.off, h.ends, spans=[(0, 8), (8, 16)])
    check_window(sd, c, h, two)
    assert ints_of(one, c.rule == "engine") == ints_of(two, c.rule == "engine")


@pytest.mark.parametrize("c", SPLIT, ids=[c.id for c in SPLIT])
def test_window_two_launch_equals_default_selection(sd, c):
    h = ww.host_side(c)
    one = run_window(sd, c, h.case, h.seed, h.off, h.ends)
    two = run_window(sd, c, h.case, h.seed, h.off, h.ends, sel="two-launch")
    print(f"[windows] {c.id}: last chunk took {one.paths[-1]} by default, {two.paths[-1]} under two-launch")
    check_window(sd, c, h, two)
    assert ints_of(one, c.rule == "engine") == ints_of(two, c.rule == "engine")


@pytest.mark.parametrize("greedy", [False, True], ids=["multinomial", "greedy"])
def test_window_stops_across_chunks(sd, greedy):
    """The stop list [ids[b, 35], ids[b, 2]] of a row b that accepts at least 36 drafts: the stop listed
    first occurs in chunk 1 only, the one listed second in chunk 0, and the return is at position 35."""
    case, seed, off, b0, stops = ww.stop_case(greedy)
    c = ww.Case("spec", "edge", case.B, case.gamma, case.V, case.dtype, not greedy)
    g = c.gamma
    proc = ref.Processor("greedy") if greedy else pw.WALK_PROC
    res = run_window(sd, c, case, seed, off, stops, proc=proc)
    lib = sd.lib
    if greedy:      # drafter == target, argmax drafts: every draft accepted, the bonus token is the argmax
        rows = [SimpleNamespace(want=g, stop_index=ref.stop_location(case.ids[b].tolist(), stops), prune_drafter=0,
                                prune_target=0, status=ww.DONE | ww.BONUS, bracket=None, close=False,
                                token=int(case.tl[b, g].float().argmax())) for b in range(c.B)]
    else:
        rows = ww.window_rows(case, "spec", seed, off, stops)
    assert rows[b0].want >= 36 and rows[b0].stop_index == ww.STOP_FIRST
    for b, r in enumerate(rows):
        assert not r.close
        n, x, st = res.n_accepted[b], res.next_token[b], res.row_status[b]
        assert not st & lib.SD_ROW_ERROR_MASK and st & lib.SD_ROW_DONE
        assert (n, res.stop_index[b]) == (r.want, r.stop_index), (b, n, res.stop_index[b], r.want, r.stop_index)
        if r.stop_index >= 0:
            assert st & lib.SD_ROW_STOP_IN_DRAFTS and x == -1, (b, hex(st), x)
            assert not st & (lib.SD_ROW_BONUS | lib.SD_ROW_RESIDUAL)
            assert (res.prune_drafter[b], res.prune_target[b]) == (0, 0)
            assert res.counts[b] == [n, n]
            continue
        assert not st & lib.SD_ROW_STOP_IN_DRAFTS
        assert bool(st & lib.SD_ROW_BONUS) == (r.want == g) and bool(st & lib.SD_ROW_RESIDUAL) == (r.want < g)
        assert (res.prune_drafter[b], res.prune_target[b]) == (r.prune_drafter, r.prune_target)
        assert res.counts[b] == [n, n + 1]
        if greedy:
            assert x == r.token
        else:
            assert r.bracket[0] <= x // pw.CHUNK_WIDTH <= r.bracket[1]
            if r.want < g:
                assert float(case.P[b, r.want, x]) > float(case.Q[b, r.want, x])
    assert res.stop_index[b0] == ww.STOP_FIRST
    assert res.status_or == 0 and res.words == 0
    print(f"[windows] stops {'greedy' if greedy else 'multinomial'}: row {b0} stops at {res.stop_index[b0]}; "
          f"stop_index = {res.stop_index}")
