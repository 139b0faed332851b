"""sd_ngram_verify under SD_NOISE_PHILOX against the host model of tests/ngram_philox_ref.py: the Philox
branch of k_ngram_rows (one block per four elements, sites 8 + segment, compare segment i and final
segment i + 1 or γ'), row_base, batches above 1, and the chunked form for γ' > 32.

Every case runs at a quiet Philox offset chosen on the host (ngram_philox_ref.quiet_offset: no draw that
the walks reach has its runner-up's score within TAU = 2^-4 of the winner's), so the device must equal
the model on every row: n_accepted, next_token, stop_index, prune_target and row_status exactly
(a nucleus row may carry SD_ROW_NUCLEUS_INEXACT, the threshold search's note that a kept probability
lies below its accumulator's ulp — informational, set from the device's own sums, and such a row is
held to the same outputs, as tests/test_gpu_parity.py holds it), words_used 0, and the filler ids
against the oracle's top-k (values; a row whose logits an fp32 exponent cannot tell apart is compared
by value within row_edges.RANK_CLOSE_RTOL, as test_gpu_row_edges.py does).  Nothing is skipped.
tests/test_ngram_philox_cpu.py proves the quiet offsets and what the walks cover.

TAU is a condition on the inputs: the device rounds E and the quotient to the rows' dtype (<= 2^-8 in
bf16) and takes E from the fp32 fast logarithm, whose error this project measures nowhere else; each
test prints the smallest winner E and the smallest top-two gap among the draws it compared.
"""
from types import SimpleNamespace

import pytest
import torch

import ngram_philox_ref as ng
import row_edges as re_
from row_edges import dt_name

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEN = SimpleNamespace(min_E=float("inf"), min_gap=float("inf"), rows=0, inexact=0)


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise)


def spec_of(sd, kind):
    p = ng.KINDS[kind]
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def call(sd, xd, drafts, kind, off, stops=(), filler_k=0, row_base=0, lo=0, hi=None):
    """ops.ngram_verify on rows [lo, hi) of xd [B, γ'+1, V] (row_base + lo); outputs on the host."""
    g = xd.shape[1] - 1
    hi = xd.shape[0] if hi is None else hi
    noise = sd.PhiloxNoise(seed=ng.NOISE_SEED, offset=off)
    status_or = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = sd.ops.ngram_verify([xd[lo:hi, t] for t in range(g + 1)], drafts[lo:hi].to(DEV), spec_of(sd, kind), noise,
                              torch.tensor(list(stops), dtype=torch.long, device=DEV), filler_k=filler_k,
                              row_base=row_base + lo, status_or=status_or)
    assert noise.offset == off + -(-g // ng.M)            # one offset per chunk
    assert int(out.words_used) == 0 and int(status_or) == 0
    return SimpleNamespace(n=out.n_accepted.cpu().tolist(), x=out.next_token.cpu().tolist(),
                           stop=out.stop_index.cpu().tolist(), prune=out.prune_target.cpu().tolist(),
                           status=out.row_status.cpu().tolist(),
                           filler=None if out.filler_ids is None else out.filler_ids.cpu())


def check_rows(sd, res, rows, kind, label):
    inexact = sd.lib.SD_ROW_NUCLEUS_INEXACT
    for b, r in enumerate(rows):
        st = res.status[b]
        if ng.KINDS[kind].kind == "nucleus" and st & inexact:      # informational (module docstring); counted
            st &= ~inexact
            SEEN.inexact += 1
        got = (res.n[b], res.x[b], res.stop[b], res.prune[b], st)
        assert got == (r.n, r.x, r.stop_index, r.prune_target, r.status), (label, b, got, vars(r))
        SEEN.min_E, SEEN.min_gap, SEEN.rows = min(SEEN.min_E, r.min_E), min(SEEN.min_gap, r.min_gap), SEEN.rows + 1


def check_filler(res, x, P, K, label):
    """ids [B, γ'+1, K] against the oracle's top-k of every row (test_gpu_row_edges.py::test_ngram_verify_step)."""
    if not K:
        assert res.filler is None
        return
    p = torch.from_numpy(P).float()
    B, rows, V = p.shape
    assert tuple(res.filler.shape) == (B, rows, K)
    for b in range(B):
        for i in range(rows):
            ids = res.filler[b, i]
            assert len(set(ids.tolist())) == K and 0 <= int(ids.min()) and int(ids.max()) < V, (label, b, i, ids)
            if re_.rank_close(x[b, i]):
                torch.testing.assert_close(p[b, i][ids], p[b, i].topk(K).values, rtol=re_.RANK_CLOSE_RTOL, atol=0)
                continue
            assert torch.equal(p[b, i][ids], p[b, i].topk(K).values), (label, b, i, ids, p[b, i].topk(K))


def report(label, rows):
    e = min(r.min_E for r in rows)
    gap = min(r.min_gap for r in rows)
    print(f"[ngram-philox] {label}: n = {[r.n for r in rows]}, smallest winner E = {e:.3g}, smallest top-two gap = {gap:.3g}")


@pytest.mark.parametrize("B,g,V,dtype", ng.STEP_SHAPES, ids=[f"B{B}-g{g}-V{V}-{dt_name(d)}" for B, g, V, d in ng.STEP_SHAPES])
def test_ngram_step_against_host_model(sd, B, g, V, dtype):
    case = ng.ngram_case(*ng.step_key(B, g, V, dtype))
    xd = case.x.to(DEV)
    for kind in ng.KINDS:
        for row_base in ng.ROW_BASES:
            _, P, off, rows = ng.step_host(B, g, V, dtype, kind, row_base)
            for K in ng.FILLER_KS:
                label = f"{kind}-base{row_base}-k{K}"
                res = call(sd, xd, case.drafts, kind, off, filler_k=K, row_base=row_base)
                check_rows(sd, res, rows, kind, label)
                check_filler(res, case.x, P, K, label)
            report(f"B{B} g{g} V{V} {dt_name(dtype)} {kind} base{row_base} off{off}", rows)


@pytest.mark.parametrize("layout", ["packed", "shifted"])
@pytest.mark.parametrize("dtype", [ng.BF16, ng.F32], ids=dt_name)
def test_ngram_step_row_layouts(sd, dtype, layout):
    """V = 2049 rows inside a NaN buffer: packed (unaligned row starts) and shifted by one element."""
    B, g, V = 5, 8, 2049
    case = ng.ngram_case(*ng.step_key(B, g, V, dtype))
    xd = re_.place(case.x, layout, float("nan"), DEV)
    for kind in ng.KINDS:
        _, P, off, rows = ng.step_host(B, g, V, dtype, kind, 1000)
        res = call(sd, xd, case.drafts, kind, off, filler_k=3, row_base=1000)
        check_rows(sd, res, rows, kind, f"{layout}-{kind}")
        check_filler(res, case.x, P, 3, f"{layout}-{kind}")


@pytest.mark.parametrize("kind", ng.SHARD_KINDS)
def test_ngram_row_shards_equal_one_call(sd, kind):
    """B = 6 as rows [0, 3) + [3, 6) with row_base = the shard's first row: the one call, and the model."""
    case, P, off, rows = ng.shard_host(kind)
    base = ng.SHARD_ROW_BASE
    xd = case.x.to(DEV)
    one = call(sd, xd, case.drafts, kind, off, filler_k=3, row_base=base)
    check_rows(sd, one, rows, kind, f"one-{kind}")
    for lo, hi in ((0, 3), (3, 6)):
        part = call(sd, xd, case.drafts, kind, off, filler_k=3, row_base=base, lo=lo, hi=hi)
        check_rows(sd, part, rows[lo:hi], kind, f"shard{lo}-{kind}")
        assert (part.n, part.x, part.status) == (one.n[lo:hi], one.x[lo:hi], one.status[lo:hi])
        assert torch.equal(part.filler, one.filler[lo:hi])
    report(f"shards {kind} off{off}", rows)


@pytest.mark.parametrize("kind", ng.STOP_KINDS)
def test_ngram_stop_among_accepted_drafts(sd, kind):
    """The stop list [drafts[b][2], drafts[b][0]]: next_token -1, STOP_IN_DRAFTS, the first-listed stop's
    position; the other rows as the model says."""
    case, P, off, rows, b, stops = ng.step_stop_case(kind)
    res = call(sd, case.x.to(DEV), case.drafts, kind, off, stops=stops, filler_k=3)
    check_rows(sd, res, rows, kind, f"stops-{kind}")
    assert res.stop[b] == 2 and res.x[b] == -1 and res.status[b] & sd.lib.SD_ROW_STOP_IN_DRAFTS
    check_filler(res, case.x, P, 3, f"stops-{kind}")


CHUNKED = [(g, V, dtype, kind) for g, V, dtype in ng.CHUNK_SHAPES for kind in ng.CHUNK_KINDS]


@pytest.mark.parametrize("g,V,dtype,kind", CHUNKED, ids=[f"g{g}-V{V}-{dt_name(d)}-{k}" for g, V, d, k in CHUNKED])
def test_ngram_chunked_window(sd, g, V, dtype, kind):
    """γ' = 33, 40 at B = 3: two chunks, two offsets; rows that mismatch at 31, at 32, inside chunk 1 and
    not at all; the filler ids of every row, the chunk-boundary row included; a stop in chunk 1."""
    case, P, off, rows = ng.chunk_host(g, V, dtype, kind)
    xd = case.x.to(DEV)
    res = call(sd, xd, case.drafts, kind, off, filler_k=3)
    check_rows(sd, res, rows, kind, f"chunked-{kind}")
    check_filler(res, case.x, P, 3, f"chunked-{kind}")
    report(f"chunked g{g} V{V} {dt_name(dtype)} {kind} off{off}", rows)
    sc = ng.chunk_stop_case(g, V, dtype, kind)
    if sc is not None:
        case, P, off, rows, b, stops = sc
        res = call(sd, xd, case.drafts, kind, off, stops=stops, filler_k=3)
        check_rows(sd, res, rows, kind, f"chunked-stops-{kind}")
        assert res.stop[b] == 33 and res.x[b] == -1 and res.status[b] & sd.lib.SD_ROW_STOP_IN_DRAFTS
        check_filler(res, case.x, P, 3, f"chunked-stops-{kind}")


def test_report_smallest_winner_and_gap():
    """(runs last) The smallest winner E and top-two gap over every draw this file compared."""
    print(f"[ngram-philox] {SEEN.rows} rows compared ({SEEN.inexact} flagged SD_ROW_NUCLEUS_INEXACT); smallest winner E = {SEEN.min_E:.3g}, "
          f"smallest top-two gap = {SEEN.min_gap:.3g} (TAU = {ng.TAU})")
    assert SEEN.min_gap >= ng.TAU
