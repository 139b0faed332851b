"""The host side of tests/test_gpu_ngram_philox.py without a GPU: the model's draws are distributed as p,
every GPU case has a quiet Philox offset (no draw that its walks reach is close), the grid's walks
include n = 0, 0 < n < γ' and n = γ', the stop cases stop, the chunked cases cross drafts 31 / 32 — and
specdec_amd/chunked.py's n-gram combination, run on CPU tensors at B = 3 with the chunk calls answered by
the one-step model, returns the window model's result bit for bit.
"""
import collections

import numpy as np
import pytest
import torch

import ngram_philox_ref as ng
import philox_ref as ph
import specdec_amd  # noqa: F401
from specdec_amd import _lib, ops
from specdec_amd.noise import PhiloxNoise
from test_gpu_perfmode import chi2_check


def test_constants_are_the_library_s():
    assert ng.M == _lib.SD_MAX_GAMMA
    assert (ng.DONE, ng.STOP_IN_DRAFTS, ng.FINISHED, ng.BONUS, ng.FALLBACK_P) == (
        _lib.SD_ROW_DONE, _lib.SD_ROW_STOP_IN_DRAFTS, _lib.SD_ROW_FINISHED, _lib.SD_ROW_BONUS, _lib.SD_ROW_FALLBACK_P)


def test_exp1_words_layout():
    """Element j reads word j & 3 of block j >> 2 of its own site; u is (w >> 8)·2^-24 + 2^-25 in fp32."""
    seed, off, row, site = 77, (1 << 33) + 5, 1003, 8 + 6
    E, u = ph.exp1_words(seed, off, row, site, 11)
    for j in range(11):
        w = int(ph.block(seed, off, row, site, j >> 2)[j & 3])
        want = np.float32(w >> 8) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
        assert u[j] == want and E[j] == -np.log(np.float64(want))
    assert not np.array_equal(E, ph.exp1_words(seed, off, row, site + 1, 11)[0])
    assert not np.array_equal(E, ph.exp1_words(seed, off + 1, row, site, 11)[0])
    assert not np.array_equal(E, ph.exp1_words(seed, off, row + 1, site, 11)[0])


def test_model_draws_are_distributed_as_p():
    V, n = 64, 4096
    p = torch.softmax(torch.randn(V, generator=torch.Generator().manual_seed(3)).double() * 2, 0).numpy()
    toks = [ng.draw(p, ph.exp1_words(11, 4, row, ng.SITE_NGRAM + 2, V)[0])[0] for row in range(n)]
    chi2_check(toks, p, "ngram model draw")


def test_draw_flags_a_close_runner_up():
    p = np.array([0.5, 0.5, 0.0])
    assert ng.draw(p, np.array([1.0, 1.0 + ng.TAU / 2, 1e-9]))[:2][0] == 0
    assert ng.draw(p, np.array([1.0, 1.0 + ng.TAU / 2, 1e-9]))[1] < ng.TAU
    assert ng.draw(p, np.array([1.0, 2.0, 1e-9]))[1] == pytest.approx(0.5)
    assert ng.draw(p, np.array([3.0, 2.0, 1e-9]))[0] == 1          # a zero-probability token never wins
    assert ng.draw(p, np.array([1.0, 1.0, 1.0]))[0] == 0           # lowest index on equality


def test_step_grid_has_quiet_offsets_and_covers_n():
    seen = collections.Counter()
    for B, g, V, dtype in ng.STEP_SHAPES:
        for kind in ng.KINDS:
            for rb in ng.ROW_BASES:
                case, P, off, rows = ng.step_host(B, g, V, dtype, kind, rb)      # raises without a quiet offset
                assert not any(r.close for r in rows)
                for r in rows:
                    seen[(ng.KINDS[kind].stochastic, "n0" if r.n == 0 else "full" if r.n == g else "mid")] += 1
    for stoch in (False, True):
        assert all(seen[(stoch, k)] >= 8 for k in ("n0", "mid", "full")), seen
    assert {(B, g, V) for B, g, V, d in ng.STEP_SHAPES if d != ng.F16} == {
        (B, g, V) for B in (1, 5) for g in (4, 8) for V in (9, 1000, 2049, 4101)}


@pytest.mark.parametrize("kind", ng.SHARD_KINDS)
def test_shard_case_has_a_quiet_offset(kind):
    case, P, off, rows = ng.shard_host(kind)              # raises without a quiet offset
    assert case.B == ng.SHARD_B and not any(r.close for r in rows)
    assert len({r.n for r in rows[:3]}) > 1 and len({r.n for r in rows[3:]}) > 1      # both shards: walks that differ


def test_hot_token_matches_with_the_stated_probability():
    key = ng.step_key(5, 8, 2049, ng.BF16)
    case, P = ng.ngram_case(*key), ng.case_probs(key, "multi_t1")
    ph_ = [P[b, i, case.hot[b, i]] for b in range(5) for i in range(8)]
    assert 0.6 <= min(ph_) and max(ph_) <= 0.9


@pytest.mark.parametrize("kind", ng.STOP_KINDS)
def test_stop_cases_stop(kind):
    case, P, off, rows, b, stops = ng.step_stop_case(kind)
    assert not any(r.close for r in rows)
    assert rows[b].stop_index == 2 and rows[b].x == -1 and rows[b].status == ng.DONE | ng.STOP_IN_DRAFTS
    assert any(r.stop_index < 0 for r in rows)


def test_chunked_cases_cross_the_chunk_edge():
    ns = collections.Counter()
    stops_seen = 0
    for g, V, dtype in ng.CHUNK_SHAPES:
        for kind in ng.CHUNK_KINDS:
            case, P, off, rows = ng.chunk_host(g, V, dtype, kind)
            assert not any(r.close for r in rows)
            for r in rows:
                ns[(kind, "31" if r.n == 31 else "32" if r.n == 32 else "full" if r.n == g else
                    "inside" if r.n > 32 else "early")] += 1
            sc = ng.chunk_stop_case(g, V, dtype, kind)
            if sc is not None:
                assert sc[3][sc[4]].stop_index == 33 and sc[3][sc[4]].x == -1
                stops_seen += 1
    for kind in ng.CHUNK_KINDS:
        assert all(ns[(kind, k)] >= 1 for k in ("31", "32", "inside", "full")), ns
    assert stops_seen >= 2


# ---------------------------------------------------------------- the combination on CPU tensors
def topk_ids(P, k):
    """[..., k] ids of the k largest probabilities, value descending, lowest index first."""
    order = np.lexsort((np.broadcast_to(np.arange(P.shape[-1]), P.shape), -P), axis=-1)
    return torch.from_numpy(order[..., :k].copy())


def make_stub(case, P, kind, seed, calls):
    starts = {case.x[:, t].data_ptr(): t for t in range(case.gamma + 1)}
    stoch = ng.KINDS[kind].stochastic

    def stub(target_rows, draft_tokens, proc, noise, stop_tokens=None, filler_k=0, sync_noise=True, row_base=0,
             status_or=None):
        c = starts[target_rows[0].data_ptr()]
        gk = len(target_rows) - 1
        assert gk <= ng.M and torch.equal(draft_tokens, case.drafts[:, c:c + gk])
        off = noise.next_offset()
        calls.append((c, gk, off))
        stops = [int(t) for t in stop_tokens.tolist()] if stop_tokens is not None else []
        rows = ng.ngram_rows(P[:, c:c + gk + 1], case.drafts[:, c:c + gk].tolist(), stoch, seed, off, row_base, stops)
        i32 = lambda f: torch.tensor([getattr(r, f) for r in rows], dtype=torch.int32)      # noqa: E731
        return ops.NgramOut(i32("n"), torch.tensor([r.x for r in rows], dtype=torch.long), i32("prune_target"),
                            i32("stop_index"), i32("status"), topk_ids(P[:, c:c + gk + 1], filler_k) if filler_k else None,
                            torch.zeros(1, dtype=torch.long))

    return stub


COMBOS = [(g, V, dtype, kind, stops) for g, V, dtype in ng.CHUNK_SHAPES for kind in ng.CHUNK_KINDS
          for stops in (False, True)]


@pytest.mark.parametrize("g,V,dtype,kind,with_stops", COMBOS,
                         ids=[f"g{g}-V{V}-{kind}{'-stops' if s else ''}" for g, V, _, kind, s in COMBOS])
def test_ngram_chunk_combination(monkeypatch, g, V, dtype, kind, with_stops):
    stops = []
    case, P, off, want = ng.chunk_host(g, V, dtype, kind)
    if with_stops:
        sc = ng.chunk_stop_case(g, V, dtype, kind)
        if sc is None:       # no row reaches draft 33: a stop in chunk 0 and the listed-first rule across rows
            b = next(b for b, r in enumerate(want) if r.n >= 3)
            stops = [int(case.drafts[b, 2]), int(case.drafts[b, 0])]
            off, want = ng.quiet_offset(P, case.drafts.tolist(), ng.KINDS[kind].stochastic, 0, stops, limit=64)
        else:
            case, P, off, want, b, stops = sc
        assert want[b].stop_index >= 0
    calls = []
    real = ops.ngram_verify
    monkeypatch.setattr(ops, "ngram_verify", make_stub(case, P, kind, ng.NOISE_SEED, calls))
    noise = PhiloxNoise(seed=ng.NOISE_SEED, offset=off)
    spec = ops.ProcSpec(ng.KINDS[kind].kind, 1.0, 0, 1.0)
    status_or = torch.zeros(1, dtype=torch.int32)
    K = 3
    out = real([case.x[:, t] for t in range(g + 1)], case.drafts, spec, noise, torch.tensor(stops, dtype=torch.long),
               filler_k=K, status_or=status_or)
    assert calls == [(0, 32, off), (32, g - 32, off + 1)] and noise.offset == off + 2
    for b, r in enumerate(want):
        got = (int(out.n_accepted[b]), int(out.next_token[b]), int(out.stop_index[b]), int(out.prune_target[b]),
               int(out.row_status[b]))
        assert got == (r.n, r.x, r.stop_index, r.prune_target, r.status), (b, got, vars(r))
        if r.stop_index >= 0:
            assert int(out.next_token[b]) == -1
    assert torch.equal(out.filler_ids, topk_ids(P, K))          # every row's own ids, the chunk-boundary row included
    assert int(status_or) == 0 and int(out.words_used) == 0


def test_grid_tells_segments_offsets_and_row_bases_apart():
    """What keeps the GPU comparison from passing with the wrong noise: over the B = 5 grid the final draw
    differs from the one the compare segment (n, not n + 1) would give, and the walks differ between
    row_base 0 and 1000 and between an offset and the next."""
    seg = base = nxt = 0
    for B, g, V, dtype in ng.STEP_SHAPES:
        if B != 5 or dtype == ng.F16:
            continue
        case, P, off, rows = ng.step_host(B, g, V, dtype, "multi_t1", 0)
        for b, r in enumerate(rows):
            if r.n < g:
                seg += ng.draw(P[b, r.n], ph.exp1_words(ng.NOISE_SEED, off, b, ng.SITE_NGRAM + r.n, V)[0])[0] != r.x
        key = lambda rs: [(r.n, r.x) for r in rs]      # noqa: E731
        drafts = case.drafts.tolist()
        base += key(rows) != key(ng.ngram_rows(P, drafts, True, ng.NOISE_SEED, off, 1000))
        nxt += key(rows) != key(ng.ngram_rows(P, drafts, True, ng.NOISE_SEED, off + 1, 0))
    assert seg >= 8 and base >= 8 and nxt >= 8, (seg, base, nxt)
