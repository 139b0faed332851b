"""The PHILOX draws of sd_sample — k_draw_lean, k_draw and k_draw_nuc — token by token against the fp64
host model that replays each draw on the same Philox words (tests/draw_ref.py: the rules, the derived
tolerances, the checker; tests/draw_cases.py: the shapes and row values; tests/test_draw_ref_cpu.py: the
model's own distribution tests, the mutants the checker rejects and the slack cap).

Every row of every call must return the model's token.  A token that differs must pass the interval test
on the same uniform (k_draw's span pick and every in-span pick), the key test (k_draw_lean's span race) or
be the outcome of a keep decision inside the device's rounding (k_draw_nuc), and the model must show the
close call too; at most 2 % of a case's rows may be close calls.  Every case asserts the kernel it ran
(_lib.last_sample_path()).  Close calls go to parity_stats.DRAW_CLOSE_CALLS; each case prints the largest
share of a slack its rows used.

token_prob (k_draw's 16-bit cases): round_dt of the fp64 processed probability of the returned token, or
its neighbour in the row dtype.  The fp32 cases ask for no token_prob: one fp32 step is finer than the
rounding of the row's fp32 normaliser (tests/test_gpu_draw.py holds those to 2e-6).
"""
import contextlib

import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_ref as dr
import row_edges as re_
from parity_stats import DRAW_CLOSE_CALLS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def sd():
    from types import SimpleNamespace
    from specdec_amd import PhiloxNoise, _lib, get_poll_policy, ops, set_poll_policy
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, get_poll_policy=get_poll_policy,
                           set_poll_policy=set_poll_policy)


def spec_of(sd, c):
    return sd.ops.ProcSpec(c.proc, c.T, c.top_k, c.top_p)


def hold(c, what, rows):
    """rows: (label, tables, model, token, check) of every (offset, row) of the case.  Asserts the checker's
    verdicts, that the model shows every close call, and the cap; prints the slack used."""
    n = closes = 0
    worst = 0.0
    for label, tb, m, tok, check in rows:
        ok, close, used, why = check(tb, m, tok)
        assert ok, (c.id, label, why)
        if tok != m.token:
            assert m.close or m.edge, (c.id, label, "the model shows no close call", why)
        if close:
            closes += 1
            DRAW_CLOSE_CALLS.append(f"{what} {c.id} {label}: {why or 'decision within tolerance; tokens equal'}")
        worst = max(worst, used)
        inner, outer = dr.slack_shares(tb)
        assert inner <= dr.SLACK_CAP and outer <= dr.SLACK_CAP, (c.id, label, inner, outer)
        n += 1
    print(f"[draw-exact] {c.id}: rows={n} close={closes} largest slack share used={worst:.3g}")
    assert closes <= dr.CLOSE_CAP * n, (c.id, closes, n)
    return closes, worst


def valid(sd, st):
    st = st.cpu()
    assert bool(((st & sd.lib.SD_ROW_DONE) != 0).all()) and not bool((st & sd.lib.SD_ROW_ERROR_MASK).any()), st.tolist()


# ---------------------------------------------------------------- k_draw_lean
@pytest.mark.parametrize("c", [c for c in dc.lean_cases() if c.mode in ("plain", "counter")], ids=lambda c: c.id)
def test_lean_draw_returns_the_models_token(sd, c):
    x, kinds = dc.case_rows(c)
    rows = dc.place(x, c.layout, DEV)
    assert re_.rows_aligned(rows)
    spec = spec_of(sd, c)
    toks = []
    old = sd.get_poll_policy()
    try:
        if c.mode == "counter":                 # no in-launch polling: the arrival counter path
            sd.set_poll_policy(False, old[1])
        with sd.lib.option(sd.lib.SD_OPT_DRAW_SPAN, c.pin) if c.pin else contextlib.nullcontext():
            for off, rb in zip(c.offsets, c.row_bases):
                tok, _, st = sd.ops.sample_rows(rows, spec, sd.PhiloxNoise(seed=c.noise_seed, offset=off), row_base=rb)
                assert sd.lib.last_sample_path() == sd.lib.SD_PATH_SAMPLE_DRAW_LEAN, sd.lib.PATH_NAMES.get(sd.lib.last_sample_path())
                valid(sd, st)
                toks.append(tok.cpu().tolist())
    finally:
        sd.set_poll_policy(*old)
    nst = dr.lean_nst(c.B, c.pin)
    tabs = [dr.lean_tables(x[r], c.dtype, nst) for r in range(c.B)]
    hold(c, "k_draw_lean", ((f"off={off} row={r} ({kinds[r]})", tabs[r], dr.lean_row(tabs[r], c.noise_seed, off, rb + r),
                             toks[i][r], dr.check_lean)
                            for i, (off, rb) in enumerate(zip(c.offsets, c.row_bases)) for r in range(c.B)))


def test_lean_draw_graph_replays_follow_the_device_offset(sd):
    """One captured draw replayed three times with advance_device(1) between the replays: replay k is the
    model's draw at offset + k."""
    c = next(c for c in dc.lean_cases() if c.mode == "graph")
    x, kinds = dc.case_rows(c)
    rows = dc.place(x, c.layout, DEV)
    spec = spec_of(sd, c)
    off, rb = c.offsets[0], c.row_bases[0]
    offset_dev = torch.zeros(1, dtype=torch.long, device=DEV)
    out = torch.full((c.B,), -7, dtype=torch.long, device=DEV)
    status = []

    def call():
        _, _, st = sd.ops.sample_rows(rows, spec, sd.PhiloxNoise(seed=c.noise_seed, offset=off, offset_dev=offset_dev),
                                      tokens_out=out, row_base=rb)
        return st

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call()                                   # the workspace exists before the capture
        with torch.cuda.graph(graph, stream=stream):
            status.append(call())
    torch.cuda.current_stream().wait_stream(stream)
    assert sd.lib.last_sample_path() == sd.lib.SD_PATH_SAMPLE_DRAW_LEAN
    noise = sd.PhiloxNoise(seed=c.noise_seed, offset=off, offset_dev=offset_dev)
    toks = []
    for k in range(3):
        out.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        valid(sd, status[0])
        toks.append(out.cpu().tolist())
        noise.advance_device(1)
    assert int(offset_dev) == 3
    tabs = [dr.lean_tables(x[r], c.dtype, dr.lean_nst(c.B)) for r in range(c.B)]
    hold(c, "k_draw_lean", ((f"replay={k} row={r} ({kinds[r]})", tabs[r], dr.lean_row(tabs[r], c.noise_seed, off + k, rb + r),
                             toks[k][r], dr.check_lean) for k in range(3) for r in range(c.B)))
    assert toks[0] != toks[1] and toks[1] != toks[2]


# ---------------------------------------------------------------- k_draw
@pytest.mark.parametrize("c", dc.draw_cases(), ids=lambda c: c.id)
def test_draw_returns_the_models_token(sd, c):
    x, kinds = dc.case_rows(c)
    rows = dc.place(x, c.layout, DEV)
    if c.layout == "general":
        assert rows.data_ptr() % 16 == 2
    spec = spec_of(sd, c)
    has_keep = c.proc != "multinomial"
    keep = torch.zeros(c.B, 4, dtype=torch.int32, device=DEV) if has_keep else None
    stats = torch.empty(c.B, 2, dtype=torch.float32, device=DEV) if has_keep else None    # keeps come with the stats
    toks, probs, keeps = [], [], []
    for off, rb in zip(c.offsets, c.row_bases):
        tok, prob, st = sd.ops.sample_rows(rows, spec, sd.PhiloxNoise(seed=c.noise_seed, offset=off), row_base=rb,
                                           want_prob=c.want_prob, row_stats_out=stats, row_keep_out=keep)
        assert sd.lib.last_sample_path() == sd.lib.SD_PATH_SAMPLE_DRAW, sd.lib.PATH_NAMES.get(sd.lib.last_sample_path())
        valid(sd, st)
        toks.append(tok.cpu().tolist())
        probs.append(prob.cpu() if c.want_prob else None)
        keeps.append(keep.cpu().numpy().copy() if has_keep else None)
    if has_keep:        # the keep predicate is a function of the row alone
        assert all(np.array_equal(k, keeps[0]) for k in keeps)
    nst = dr.draw_nst(c.B, c.V, c.dtype)
    tabs, skipped = [], 0
    for r in range(c.B):
        kp = dr.keep_of(keeps[0][r]) if has_keep else None
        if kp is not None and kp[2] & sd.lib.SD_ROW_NUCLEUS_INEXACT:       # a cut among p < 2^-17: not modelled
            tabs.append(None)
            skipped += 1
            continue
        tabs.append(dr.draw_tables(x[r], c.dtype, c.T, kp, nst))
    assert skipped * 8 <= c.B, (c.id, skipped)
    if skipped:
        print(f"[draw-exact] {c.id}: {skipped} of {c.B} rows flagged SD_ROW_NUCLEUS_INEXACT, skipped")
    hold(c, "k_draw", ((f"off={off} row={r} ({kinds[r]})", tabs[r], dr.draw_row(tabs[r], c.noise_seed, off, rb + r),
                        toks[i][r], dr.check_draw)
                       for i, (off, rb) in enumerate(zip(c.offsets, c.row_bases)) for r in range(c.B) if tabs[r] is not None))
    if c.want_prob:
        for i in range(len(c.offsets)):
            live = [r for r in range(c.B) if tabs[r] is not None]
            want = torch.tensor([dr.token_prob(tabs[r], toks[i][r], c.dtype) for r in live], dtype=torch.float32).to(c.dtype)
            got = probs[i][live]
            assert torch.equal(got.to(c.dtype).float(), got), (c.id, "token_prob is not a value of the row dtype")
            near = re_.within_one_ulp(got.to(c.dtype), want)
            assert bool(near.all()), (c.id, i, got[~near].tolist(), want[~near].float().tolist())


# ---------------------------------------------------------------- k_draw_nuc
@pytest.mark.parametrize("c", dc.nuc_cases(), ids=lambda c: c.id)
def test_nucleus_draw_returns_the_models_token(sd, c):
    x, kinds = dc.case_rows(c)
    rows = x.to(DEV)
    spec = spec_of(sd, c)
    toks = []
    for off, rb in zip(c.offsets, c.row_bases):
        tok, prob, st = sd.ops.sample_rows(rows, spec, sd.PhiloxNoise(seed=c.noise_seed, offset=off), row_base=rb)
        assert prob is None
        assert sd.lib.last_sample_path() == sd.lib.SD_PATH_SAMPLE_NUCLEUS, sd.lib.PATH_NAMES.get(sd.lib.last_sample_path())
        valid(sd, st)
        assert not bool((st.cpu() & sd.lib.SD_ROW_NUCLEUS_INEXACT).any())
        toks.append(tok.cpu().tolist())
    tabs = [dr.nuc_tables(x[r], c.dtype, c.T, c.top_p) for r in range(c.B)]
    models = [[dr.nuc_row(tabs[r], c.noise_seed, off, rb + r) for r in range(c.B)] for off, rb in zip(c.offsets, c.row_bases)]
    rounds = max(m.rounds for ms in models for m in ms)
    later = sum(m.first_k > 0 or m.rounds > 1 for ms in models for m in ms)
    print(f"[draw-exact] {c.id}: the model needed up to {rounds} rounds, {later} rows a proposal after their first")
    # the seed's condition (tests/test_draw_ref_cpu.py proves it without a GPU): rounds beyond the first at
    # top_p = 0.5; at 0.9 a second round has probability <= 1e-4 per draw, so a later proposal of round 0
    assert rounds >= 2 if c.top_p == 0.5 else later > 0
    hold(c, "k_draw_nuc", ((f"off={off} row={r} ({kinds[r]})", tabs[r], models[i][r], toks[i][r], dr.check_nuc)
                           for i, (off, rb) in enumerate(zip(c.offsets, c.row_bases)) for r in range(c.B)))
