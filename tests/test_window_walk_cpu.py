"""The host side of tests/test_gpu_philox_windows.py without a GPU: the pinned offsets cover what the
GPU cases claim (window_walk.coverage, for exactly the cases and offsets that file runs), and the
device-side combination of specdec_amd/chunked.py is run on CPU tensors at B = 16 with the chunk calls
answered by the ONE-CALL host model (perf_walk.host_rows on the chunk's slice with the call's offset):
ops.verify must then return exactly what the one-window model (window_walk.window_rows) states.  Both
sides are the same host arithmetic, so the comparison is bit for bit.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import perf_walk as pw
import philox_ref as ph
import specdec_amd  # noqa: F401
import window_walk as ww
from oracle import specdec_ref as ref
from specdec_amd import _lib, ops
from specdec_amd.noise import PhiloxNoise

STEP, PAD, ACC0 = 4, 4, 7


def test_chunk_width_is_the_library_s():
    assert ww.M == _lib.SD_MAX_GAMMA
    assert (ww.DONE, ww.STOP_IN_DRAFTS, ww.FINISHED, ww.RESIDUAL, ww.BONUS, ww.FALLBACK_P) == (
        _lib.SD_ROW_DONE, _lib.SD_ROW_STOP_IN_DRAFTS, _lib.SD_ROW_FINISHED, _lib.SD_ROW_RESIDUAL,
        _lib.SD_ROW_BONUS, _lib.SD_ROW_FALLBACK_P)


def test_window_pivots():
    assert ww.window_pivots(33) == [0, 3, 4, 7, 8, 31, 32]
    assert ww.window_pivots(40) == [0, 3, 4, 7, 8, 31, 32, 33, 39]
    assert ww.window_pivots(64) == [0, 3, 4, 7, 8, 31, 32, 33, 63]
    assert ww.window_pivots(70) == [0, 3, 4, 7, 8, 31, 32, 33, 63, 64, 69]
    assert pw.pivots(40) == [0, 3, 4, 7, 8, 39]                      # existing callers: unchanged
    assert ww.window_cycle(40) == (39, 31, 32, 33, 0, 3, 4, 7, 8)
    cyc8 = ww.window_cycle(40, 8)          # seven active rows, seven conditions that need their own row
    assert cyc8 == (39, 31, 32, 0, 33, 39, 32, 3) and set(cyc8) <= set(ww.window_pivots(40))
    assert [k for b, k in enumerate(cyc8) if pw.active_mask(8)[b] and k >= 31] == [39, 31, 32, 33, 39, 32]
    case = ww.case_inputs(ww.Case("spec", "edge", 16, 40, 2048, ww.BF16, True))
    assert case.k == [ww.window_cycle(40)[b % 9] for b in range(16)]


def test_window_uniforms_take_the_chunk_s_offset():
    seed, off, rb = 99, 1 << 33, 1003
    for i in (0, 31, 32, 33, 63, 64, 69):
        assert ww.accept_uniform(seed, off, rb, i) == ph.accept_uniform(seed, off + i // 32, rb, i % 32)
    assert ww.accept_uniform(seed, off, rb, 32) != ph.accept_uniform(seed, off, rb, 32)


@pytest.mark.parametrize("c", ww.CASES, ids=[c.id for c in ww.CASES])
def test_gpu_window_cases_cover_what_they_claim(c):
    assert c.key in ww.OFFSETS
    assert ww.coverage(c, ww.host_side(c)) == []


def test_gpu_grid_is_the_issue_s():
    keys = {(c.rule, c.B, c.gamma, c.V, c.dtype, c.draws, c.row_base) for c in ww.CASES}
    for rule in ("spec", "engine"):
        assert {(rule, 16, 33, 2049, ww.F16, False, 0), (rule, 16, 40, 2048, ww.BF16, True, 0),
                (rule, 16, 40, 2048, ww.BF16, False, 0), (rule, 16, 40, 2048, ww.BF16, True, 1000),
                (rule, 16, 40, 2048, ww.BF16, False, 1000), (rule, 16, 64, 2048, ww.BF16, True, 0),
                (rule, 16, 70, 1000, ww.F32, False, 0), (rule, 8, 40, 4101, ww.BF16, True, 7)} <= keys
    assert ("spec", 1, 40, 4096, ww.BF16, True, 0) in keys
    for g in (40, 70):
        assert {c.kind for c in ww.CASES if c.gamma == g and c.B == 16 and not c.row_base} == {"edge", "long"}


@pytest.mark.parametrize("greedy", [False, True])
def test_stop_case_puts_the_first_listed_stop_in_chunk_1(greedy):
    case, seed, off, b, stops = ww.stop_case(greedy)
    ids = case.ids[b].tolist()
    assert ids.index(stops[0]) == 35 and ids.index(stops[1]) == 2 and stops[0] != stops[1]
    assert ref.stop_location(ids[:36], stops) == 35 and ref.stop_location(ids[:35], stops) == 2
    if not greedy:
        rows = ww.window_rows(case, "spec", seed, off, stops)
        assert rows[b].want >= 36 and rows[b].stop_index == 35 and not any(r.close for r in rows)
        assert any(r.stop_index < 0 and r.rejected for r in rows) and any(2 < r.want < 35 for r in rows)


# ---------------------------------------------------------------- the combination on CPU tensors
def nan_eq(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def make_stub(case, rule, seed, ends, calls):
    """ops.verify for one chunk on CPU tensors, answered from the one-call host model."""
    engine = rule == "engine"
    starts = {case.tl[:, t].data_ptr(): t for t in range(case.gamma + 1)}

    def stub(target_rows, draft_rows, draft_tokens, rule_id, target_proc, draft_proc, noise, stop_tokens=None,
             skip_sample_adjustment=False, draft_is_probs=False, active=None, engine_state=None, sync_noise=True,
             prof_events=None, row_base=0, draft_row_stats=None, draft_row_keep=None, status_or=None,
             row_counts=None):
        c = starts[target_rows[0].data_ptr()]
        gk = len(draft_rows)
        B = target_rows[0].shape[0]
        assert B == case.B and gk <= ww.M and len(target_rows) == (gk if engine else gk + 1)
        assert torch.equal(draft_tokens, case.ids[:, c:c + gk])
        off = noise.next_offset()    # a call takes the next offset
        calls.append((c, gk, off))
        sub = SimpleNamespace(gamma=gk, ids=case.ids[:, c:c + gk], P=case.P[:, c:c + gk + 1], Q=case.Q[:, c:c + gk],
                              B=B)
        act = None if active is None else [bool(a) for a in active.tolist()]
        stops = [int(t) for t in stop_tokens.tolist()] if stop_tokens is not None else []
        rows = pw.host_rows(sub, rule, seed, off, stops if engine else (), row_base, act)
        out = ops.VerifyOut(torch.zeros(B, dtype=torch.int32), torch.full((B,), -1, dtype=torch.long),
                            torch.full((B,), float("nan")), torch.zeros(B, dtype=torch.int32),
                            torch.zeros(B, dtype=torch.int32), torch.full((B,), -1, dtype=torch.int32),
                            torch.zeros(B, dtype=torch.int32), torch.zeros(1, dtype=torch.long))
        for b, r in enumerate(rows):
            if not r.active:
                continue
            out.n_accepted[b] = r.want
            st = ww.DONE
            x = -1
            stop = ref.stop_location(sub.ids[b, :r.want].tolist(), stops) if not engine else -1
            if stop >= 0:
                st |= ww.STOP_IN_DRAFTS
                out.stop_index[b] = stop
            elif r.weights is not None:
                w = (sub.P[b, r.slot].double() - sub.Q[b, r.slot].double()).clamp(min=0) if r.weights == "residual" \
                    else sub.P[b, r.slot].double()
                x = ww.inverse_cdf(w.numpy(), ph.cdf_uniform(seed, off, row_base + b))
                st |= {"residual": ww.RESIDUAL, "bonus": ww.BONUS, "p": ww.FALLBACK_P}[r.weights]
                if r.rejected:
                    out.resample_mass[b] = r.res_mass
                    if not engine:
                        out.prune_drafter[b], out.prune_target[b] = gk - r.want, gk - r.want + 1
            out.next_token[b] = x
            if engine:
                fin = r.finished or x in stops
                st |= ww.FINISHED if fin else 0
                if engine_state is not None:      # one kernel call's state update (infer_engine.py:326-336)
                    gen, step = engine_state["generated"], engine_state["step"]
                    engine_state["accepted"][b] += r.want
                    if r.rejected:
                        gen[b, step + r.want] = x
                    if r.want < gk:
                        gen[b, step + r.want + 1: step + gk] = 0
                    if fin:
                        engine_state["finished"][b] = 1
                if row_counts is not None:
                    row_counts[b] += torch.tensor([r.want, r.want + (x >= 0)])
            out.row_status[b] = st
        return out

    return stub


COMBOS = [(rule, g, kind) for rule in ("spec", "engine") for g in (33, 40, 70) for kind in ("edge", "long")]


@pytest.mark.parametrize("rule,g,kind", COMBOS, ids=[f"{r}-g{g}-{k}" for r, g, k in COMBOS])
@pytest.mark.parametrize("with_stops", [False, True], ids=["no-stops", "stops"])
def test_chunk_combination_at_batch_16(monkeypatch, rule, g, kind, with_stops):
    B, V, row_base = 16, 257, 1000
    engine = rule == "engine"
    case = pw.walk_case(kind, B, g, V, torch.float32, 11, ww.window_cycle(g) if kind == "edge" else None)
    seed, off = ww.NOISE[rule]
    off += 3
    active = pw.active_mask(B) if engine else None
    stops = []
    if with_stops and engine:    # the first offset whose free walk has a row to end at draft 31 and one in chunk 1
        off = next(o for o in range(off, off + 64) if None not in ww.window_ends(case, seed, o, row_base, active))
        stops, at31, later = ww.window_ends(case, seed, off, row_base, active)
    elif with_stops:         # listed first: a token accepted in chunk 1; second: one accepted in chunk 0
        free = ww.window_rows(case, "spec", seed, off, (), row_base)
        b = next(b for b, r in enumerate(free) if r.want > ww.M)
        stops = [int(case.ids[b, ww.M]), int(case.ids[b, 2])]
    want = ww.window_rows(case, rule, seed, off, stops, row_base, active)
    assert any(r.active and r.want < ww.M for r in want) and any(r.want >= ww.M for r in want)
    if with_stops and not engine:
        assert any(r.stop_index >= ww.M for r in want)
    check_combination(monkeypatch, case, rule, seed, off, stops, row_base, active, want)


def check_combination(monkeypatch, case, rule, seed, off, stops, row_base, active, want):
    """ops.verify over the window on CPU tensors, its chunk calls answered by the stub, against `want`."""
    B, g, engine = case.B, case.gamma, rule == "engine"
    calls = []
    real = ops.verify
    stub = make_stub(case, rule, seed, stops, calls)
    monkeypatch.setattr(ops, "verify", stub)
    noise = PhiloxNoise(seed=seed, offset=off)
    counts = torch.zeros(B, 2, dtype=torch.long)
    status_or = torch.zeros(1, dtype=torch.int32)
    n_t = g if engine else g + 1
    kw = {}
    generated0 = torch.zeros(B, STEP + g + PAD, dtype=torch.long)
    generated0[:, STEP:STEP + g] = case.ids
    if engine:
        st = dict(generated=generated0.clone(), step=STEP, finished=torch.zeros(B, dtype=torch.uint8),
                  accepted=torch.full((B,), ACC0, dtype=torch.long))
        kw = dict(active=torch.tensor(active, dtype=torch.uint8), engine_state=st)
    proc = ops.ProcSpec("multinomial", 1.0, 0, 1.0)
    out = real([case.tl[:, t] for t in range(n_t)], [case.dl[:, d] for d in range(g)], case.ids,
               _lib.SD_RULE_ENGINE if engine else _lib.SD_RULE_SPEC, proc, proc, noise,
               torch.tensor(stops, dtype=torch.long), row_base=row_base, status_or=status_or, row_counts=counts, **kw)
    assert calls == [(k * ww.M, min(ww.M, g - k * ww.M), off + k) for k in range(ww.n_chunks(g))]
    assert noise.offset == off + ww.n_chunks(g)
    for b, r in enumerate(want):
        got = (int(out.n_accepted[b]), int(out.next_token[b]), int(out.row_status[b]), int(out.stop_index[b]),
               int(out.prune_drafter[b]), int(out.prune_target[b]), float(out.resample_mass[b]))
        exp = (r.want, r.token, r.status if r.active else 0, r.stop_index, r.prune_drafter, r.prune_target,
               float(torch.tensor(r.res_mass, dtype=torch.float32)) if r.rejected and r.stop_index < 0 else math.nan)
        assert all(nan_eq(a, e) for a, e in zip(got, exp)), (b, got, exp)
        assert counts[b].tolist() == ([r.want, r.want + (r.token >= 0)] if r.active else [0, 0]), (b, counts[b])
    assert int(status_or) == 0 and int(out.words_used) == 0
    if engine:
        gen, fin, acc = ww.engine_expect(case, want, generated0, STEP, ACC0)
        assert torch.equal(st["generated"], gen) and torch.equal(st["finished"], fin) and torch.equal(st["accepted"], acc)


def test_equal_rank_stop_keeps_the_earlier_chunk_s_position(monkeypatch):
    """One stop token at draft 5 (chunk 0) and again at draft 33 (chunk 1) of a row that accepts the whole
    window: the return is at its first position, 5 (the rows before a pivot have p == q on every token,
    so the repeated token is accepted like the one it replaces)."""
    B, g, row_base = 16, 40, 1000
    base = pw.walk_case("edge", B, g, 257, torch.float32, 11, ww.window_cycle(g))
    assert base.k[0] == g - 1 and torch.equal(base.P[0, 33], base.Q[0, 33]) and float(base.Q[0, 33, base.ids[0, 5]]) > 0
    ids = base.ids.clone()
    ids[0, 33] = ids[0, 5]
    case = SimpleNamespace(tl=base.tl, dl=base.dl, ids=ids, P=base.P, Q=base.Q, B=B, gamma=g, V=base.V, dtype=base.dtype)
    seed, off = ww.NOISE["spec"]
    stops = [int(ids[0, 5])]
    want = ww.window_rows(case, "spec", seed, off, stops, row_base)
    assert want[0].want >= 34 and want[0].stop_index == 5
    check_combination(monkeypatch, case, "spec", seed, off, stops, row_base, None, want)
