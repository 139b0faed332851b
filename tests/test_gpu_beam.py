"""The device beam step (csrc/beam.hip) on the GPU: the row pass's top-k log-probs against a float64
log-softmax, the selection bit-for-bit against tests/beam_ref.py (SD_BEAM_TOPK_GIVEN), and workspace
reuse.

The log-prob bound: the reference's own ``torch.log_softmax`` in fp32 is E away from a float64
log-softmax on the golden rows (``logsoftmax_err`` of tests/golden/beam_loops.json, measured by
make_golden_base.py: 1.26e-6 on the rows of up to 4096 entries, 1.05e-5 on the 128256-entry rows —
each bounds the rows of its size here); the kernel, whose exp / log and reduction order differ from
torch's, may be max(4 E, 2 fp32 ulps at the value's magnitude) away.  For 16-bit rows the values are
equal after rounding unless the float64 value lies within that bound of a rounding boundary (a close
call); at most 1 % of the compared values may be close calls.  Tokens: the kernel's place j must hold
the float64 order's token unless the float64 values around place j lie within TWICE the bound of each
other — each of the two values may be off by the bound, so only a gap above twice the bound fixes
their order in every admissible arithmetic.
"""
import functools
import json
import os

import pytest
import torch

import beam_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "beam_loops.json")) as f:
    GOLD = json.load(f)
# torch's fp32 log_softmax drifts with the row length (its sum is longer): the figure measured on the
# goldens of up to 4096 entries bounds the rows of up to 4104, the figure over all goldens (the
# 128256-entry rows set it) the larger rows.  One figure for all would be the second, 8x looser.
E_SMALL = max(c["logsoftmax_err"] for c in GOLD.values() if c["vocab"] <= 4096)
E_REF = max(c["logsoftmax_err"] for c in GOLD.values())


def e_for(V: int) -> float:
    return E_SMALL if V <= 4104 else E_REF
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
POISON = 3.0e4   # finite in every dtype: a kernel that read it would move every log-prob


def bound_of(v64: torch.Tensor, E: float) -> torch.Tensor:
    mag = v64.abs().clamp(max=3e38).float()
    ulp = (torch.nextafter(mag, torch.tensor(float("inf"))) - mag).double()
    return torch.maximum(torch.full_like(v64, 4 * E), 2 * ulp)


def boundary_distance(v64: torch.Tensor, dtype) -> torch.Tensor:
    r = v64.to(dtype)
    inf = torch.tensor(float("inf"), dtype=dtype)
    up, dn = torch.nextafter(r, inf).double(), torch.nextafter(r, -inf).double()
    r = r.double()
    return torch.minimum((v64 - (r + up) / 2).abs(), (v64 - (r + dn) / 2).abs())


def make_rows(V: int, dtype, seed: int) -> torch.Tensor:
    """Five rows: plain; with -inf entries; maximum at the last element; flat (log-probs of distinct
    logits round to one 16-bit value, and whole spans tie at the K-th place); plain."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, V, generator=g) * 3
    x[1, torch.rand(V, generator=g) < 0.1] = float("-inf")
    x[1, V // 2] = 1.0   # never a whole row of -inf
    x[2, V - 1] = x[2].max() + 0.25
    x[3] = torch.randn(V, generator=g) * 0.5
    return x.to(dtype)


def layouts(x: torch.Tensor):
    """The rows packed, padded (row stride V + 24) and shifted by one element, inside poisoned buffers."""
    R, V = x.shape
    yield "packed", x.to(DEV)
    pad = torch.full((R, V + 24), POISON, dtype=x.dtype, device=DEV)
    pad[:, :V] = x.to(DEV)
    yield "padded", pad[:, :V]
    buf = torch.full((R * (V + 9) + 1,), POISON, dtype=x.dtype, device=DEV)
    sh = buf[1:].view(R, V + 9)[:, :V]
    sh.copy_(x.to(DEV))
    yield "shifted", sh


def check_topk(x: torch.Tensor, lp: torch.Tensor, tok: torch.Tensor, K: int, stats: dict, where: str):
    """x [R, V] CPU rows in their dtype; lp / tok the kernel's output (CPU)."""
    R, V = x.shape
    E = e_for(V)
    lp64 = torch.log_softmax(x.double(), dim=-1)
    sixteen = x.dtype != torch.float32
    for r in range(R):
        row, t, v = lp64[r], tok[r], lp[r].double()
        assert len(set(t.tolist())) == K and int(t.min()) >= 0 and int(t.max()) < V, (where, r, "ids")
        at = row[t]                                   # float64 log-prob of each reported token
        fin = torch.isfinite(at)
        assert torch.equal(torch.isinf(v) & (v < 0), ~fin), (where, r, "-inf places")
        b = bound_of(at[fin], E)
        if sixteen:
            exp_v = at.to(x.dtype).double()
            close = torch.zeros(K, dtype=torch.bool)
            close[fin] = boundary_distance(at[fin], x.dtype) < b
            stats["compared"] += K
            stats["close"] += int(close.sum())
            ok = (v == exp_v) | close
            assert bool(ok.all()), (where, r, "values", v[~ok].tolist(), exp_v[~ok].tolist())
            # a close call may move a value by one step of the dtype, never further
            step = (torch.nextafter(exp_v.to(x.dtype), torch.tensor(float("inf"), dtype=x.dtype)).double() - exp_v).abs()
            assert bool(((v - exp_v).abs()[fin] <= step[fin] + 1e-12).all()), (where, r, "close-call size")
            key = row.to(x.dtype).double()            # the order the reference sorts by: rounded values
        else:
            assert bool(((v[fin] - at[fin]).abs() <= b).all()), (where, r, "values", float((v[fin] - at[fin]).abs().max()))
            key = row
        ev, ei = beam_ref.topk_lowest_index(key, min(K + 1, V))
        gaps = torch.cat([torch.tensor([float("inf")], dtype=torch.float64), (ev[:-1] - ev[1:]).nan_to_num(nan=0.0),
                          torch.tensor([float("inf")], dtype=torch.float64)])
        for j in range(K):
            if int(t[j]) == int(ei[j]):
                continue
            # a different token only where the float64 values around place j are within the bound of
            # each other (fp32) or a close call sits in the row's top-(K+1) (16-bit)
            if sixteen:
                cand = row[ei][torch.isfinite(row[ei])]
                assert bool((boundary_distance(cand, x.dtype) < bound_of(cand, E)).any()), (where, r, j, "order")
            else:
                bj = float(bound_of(ev[j:j + 1].clamp(min=-3e38), E)[0])
                assert min(float(gaps[j]), float(gaps[j + 1])) <= 2 * bj, (where, r, j, "order")


VOCABS = ["K", 2047, 2048, 2049, 4104, 128256]


@functools.lru_cache(maxsize=None)
def run_matrix(dt: str, V):
    """One (dtype, V) cell of the matrix: every K, R and layout compared; returns (16-bit values
    compared, close calls among them).  Cached, so whichever test asks first runs it."""
    from specdec_amd import ops
    dtype = DTYPES[dt]
    stats = dict(compared=0, close=0)
    for K in (1, 3, 8, 64):
        v = K if V == "K" else V
        for R in (1, 4, 5):
            for li, name in enumerate(("packed", "padded", "shifted")):
                if v == 128256 and (name == "padded" or (R, K) not in ((4, 1), (1, 64), (4, 3), (5, 8), (5, 64))):
                    continue   # the large vocabulary once per K and R, packed and shifted
                x = make_rows(v, dtype, seed=(((v * 67 + K) * 7 + R) * 3 + li) * 16)   # fresh rows per comparison
                if v == K:
                    x[1] = x[4]   # with V == K every element is reported: keep -inf out of the tiny rows
                dev_rows = dict(layouts(x[:R]))[name]
                lp, tok = ops.beam_topk(dev_rows, K)
                check_topk(x[:R], lp.cpu(), tok.cpu(), K, stats, f"{dt} V={v} K={K} R={R} {name}")
    return stats["compared"], stats["close"]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_topk_logprobs_vs_float64(dt, V):
    compared, close = run_matrix(dt, V)
    print(f"{dt} V={V}: {compared} 16-bit values compared, {close} close calls; "
          f"E = {e_for(4096):.3e} (rows <= 4104) / {E_REF:.3e}, bound = max(4 E, 2 ulp)")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_close_calls_are_rare(dt):
    """Over every 16-bit value the whole matrix compares (its cells are run here if they have not
    been yet): at most 1 % lie within the bound of a rounding boundary.  The count depends on the
    rows and the bound, not on the kernel: a 16-bit row's log-probs share their offset from the
    rounding grid, so whole rows are close calls together and the rate swings with the seeds (0.3 %
    to 1.1 % over the seed families tried on the CPU from the float64 values alone; these seeds:
    0.26 % bf16, 0.37 % fp16)."""
    cells = [run_matrix(dt, V) for V in VOCABS]
    compared, close = sum(c[0] for c in cells), sum(c[1] for c in cells)
    print(f"{dt}: {close} close calls in {compared} compared values")
    assert compared > 0
    assert close <= 0.01 * compared


def test_bf16_ties_at_the_kth_place_are_lowest_index_first():
    from specdec_amd import ops
    V, K = 4104, 3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, V, generator=g).to(torch.bfloat16)
    tied = [3000, 100, 4000, 50, 2500]
    x[0, tied] = 9.0               # five equal maxima: the three lowest indices, in order
    x[1, 7] = 9.5
    x[1, tied] = 9.0               # one clear winner, then the tie cut at the K-th place
    lp, tok = ops.beam_topk(x.to(DEV), K)
    assert tok[0].tolist() == [50, 100, 2500]
    assert tok[1].tolist() == [7, 50, 100]
    ref_lp, ref_tok = beam_ref.logprob_topk(x, K)
    assert torch.equal(tok.cpu(), ref_tok)
    assert torch.equal(lp.cpu(), ref_lp)
    assert float(lp[0, 0]) == float(lp[0, 2])


# ------------------------------------------------------------------ selection, bit-exact
def run_select(state, top_lp, top_tok, curr, length, stops, pad):
    """The same step through tests/beam_ref.py and through sd_beam_step(SD_BEAM_TOPK_GIVEN)."""
    from specdec_amd import ops
    n, k = top_lp.shape
    ref = beam_ref.select(state, top_lp, top_tok, curr, beam_ref.length_penalty(length, 1.2, 5.0), stops, pad)
    st = ops.BeamState(state["ids"].to(DEV), state["probs"].to(DEV), state["bp"].to(DEV), state["li"].to(DEV))
    done = ops.beam_step(st, None, curr, top_k=k, length=length, alpha=1.2, min_length=5.0,
                         stop_tokens=torch.tensor(stops, dtype=torch.long, device=DEV), pad_token_id=pad,
                         topk=(top_lp.to(DEV).contiguous(), top_tok.to(DEV).contiguous()))
    assert int(done.item()) == ref["all_finished"]
    if ref["all_finished"] < 0:
        return ref, st
    assert beam_ref.bits(st.beams_probs.cpu()) == beam_ref.bits(ref["bp"])
    assert st.last_indexes.tolist() == ref["li"].tolist()
    assert torch.equal(st.input_ids.cpu(), ref["ids"])
    assert beam_ref.bits(st.probs.cpu()) == beam_ref.bits(ref["probs"])
    assert st.parent.tolist() == ref["parent"].tolist()
    return ref, st


def make_state(n, L, curr, seed, finished=(), V=1000):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (n, L), generator=g)
    ids[:, curr:] = 0
    probs = torch.full((n, L), beam_ref.F32_MIN)
    probs[:, :curr] = 1.0 - torch.rand(n, curr, generator=g) * 5
    bp = -torch.rand(n, generator=g) * 3
    li = torch.full((n,), -1, dtype=torch.long)
    for b in finished:
        li[b] = curr - 1
    return dict(ids=ids, probs=probs, bp=bp, li=li)


def make_topk(n, k, seed, V=1000):
    g = torch.Generator().manual_seed(1000 + seed)
    lp = -torch.sort(torch.rand(n, k, generator=g) * 6, dim=-1).values
    tok = torch.stack([torch.randperm(V - 3, generator=g)[:k] + 3 for _ in range(n)])
    return lp.float(), tok


def test_select_all_live():
    st = make_state(4, 12, 6, seed=1)
    run_select(st, *make_topk(4, 3, 1), curr=6, length=3, stops=[1], pad=0)


def test_select_finished_beams_win_lose_and_move():
    # beam 1 finished with the best score (moves down to slot 0), beam 2 finished with a poor one (lost)
    st = make_state(4, 12, 6, seed=2, finished=(1, 2))
    st["bp"][1], st["bp"][2] = 5.0, -50.0
    ref, _ = run_select(st, *make_topk(4, 3, 2), curr=6, length=3, stops=[1], pad=0)
    assert ref["parent"][0].tolist() == [1, -1] and [2, -1] not in ref["parent"].tolist()
    # beam 0 finished with the worst surviving score: it sorts to the last slot and reads slot 0,
    # already rewritten by a live candidate — a revival (last index -1) with that candidate's score
    st = make_state(4, 12, 6, seed=3, finished=(0,))
    st["bp"][0] = -40.0
    lp, tok = make_topk(4, 1, 3)
    ref, _ = run_select(st, lp, tok, curr=6, length=3, stops=[1], pad=0)
    assert ref["parent"][3].tolist() == [0, -1] and int(ref["li"][3]) == -1
    assert float(ref["bp"][3]) == float(ref["bp"][0])
    copy = beam_ref.select(st, lp, tok, 6, beam_ref.length_penalty(3, 1.2, 5.0), [1], 0, copy_semantics=True)
    assert int(copy["li"][3]) == 5 and float(copy["bp"][3]) == -40.0


def test_select_dedupe_drops_the_second_identical_parent():
    st = make_state(3, 10, 5, seed=4)
    st["ids"][1] = st["ids"][0]
    st["probs"][1] = st["probs"][0]
    lp, tok = make_topk(3, 2, 4)
    lp[1], tok[1] = lp[0], tok[0]
    ref, _ = run_select(st, lp, tok, curr=5, length=2, stops=[1], pad=0)
    assert 1 not in ref["parent"][:, 0].tolist()
    # a finished beam that already holds a live beam's child
    st = make_state(3, 10, 5, seed=5, finished=(0,))
    lp, tok = make_topk(3, 2, 5)
    st["ids"][0] = st["ids"][1]
    st["ids"][0, 5] = tok[1, 0]
    st["bp"][0] = -100.0
    ref, _ = run_select(st, lp, tok, curr=5, length=2, stops=[1], pad=0)
    assert [1, 0] not in ref["parent"].tolist()
    # every candidate a duplicate: fewer entries than beams, where the reference raises
    st = make_state(2, 10, 5, seed=6)
    st["ids"][1] = st["ids"][0]
    lp, tok = make_topk(2, 1, 6)
    tok[1] = tok[0]
    ref, _ = run_select(st, lp, tok, curr=5, length=2, stops=[1], pad=0)
    assert ref["all_finished"] == -1


def test_select_equal_scores_keep_generation_order():
    st = make_state(4, 10, 5, seed=7)
    st["probs"][:, 4] = -2.0
    lp, tok = make_topk(4, 3, 7)
    lp[:] = torch.tensor([-1.0, -1.0, -3.0])
    ref, _ = run_select(st, lp, tok, curr=5, length=2, stops=[1], pad=0)
    assert ref["parent"].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]


@pytest.mark.parametrize("n_stop", [1, 64])
def test_select_pad_and_stop_tokens_finish_a_beam(n_stop):
    st = make_state(4, 10, 5, seed=8)
    lp, tok = make_topk(4, 3, 8)
    stops = list(range(500, 500 + n_stop))
    tok[0, 0], tok[1, 0], tok[2, 1] = 0, stops[-1], stops[0]   # pad id, last and first listed stop
    lp[:, 0] = -0.01
    ref, _ = run_select(st, lp, tok, curr=5, length=2, stops=stops, pad=0)
    assert sorted(ref["li"].tolist()).count(5) >= 2


def test_select_single_beam_and_widest_shape():
    st = make_state(1, 8, 4, seed=9)
    run_select(st, *make_topk(1, 1, 9), curr=4, length=1, stops=[1], pad=0)
    st = make_state(64, 40, 20, seed=10, finished=(3, 17, 40, 63))
    lp, tok = make_topk(64, 16, 10)
    tok[5, 2] = 1
    run_select(st, lp, tok, curr=20, length=12, stops=[1], pad=0)
    # all beams finished: nothing is expanded, all_finished is 1
    st = make_state(3, 8, 4, seed=11, finished=(0, 1, 2))
    ref, _ = run_select(st, *make_topk(3, 2, 11), curr=4, length=1, stops=[1], pad=0)
    assert ref["all_finished"] == 1


def test_prefill_against_the_restatement():
    from specdec_amd import ops
    for dt in (torch.float32, torch.bfloat16):
        x = (torch.randn(1, 4104, generator=torch.Generator().manual_seed(3)) * 3).to(dt)
        ref0 = beam_ref.initial_state([5, 9, 2, 81], 4, 10, 0)
        ref = beam_ref.prefill(ref0, *beam_ref.logprob_topk(x, 4), 4, beam_ref.length_penalty(1, 1.2, 5.0))
        st = ops.BeamState.start([5, 9, 2, 81], 4, 10, 0, DEV)
        done = ops.beam_step(st, x.to(DEV), 4, prefill=True, length=1, stop_tokens=torch.tensor([1], device=DEV))
        assert int(done.item()) == 0
        assert torch.equal(st.input_ids.cpu(), ref["ids"])
        got, want = st.probs.cpu()[:, 4].double(), ref["probs"][:, 4].double()
        assert bool(((got - want).abs() <= bound_of(want, E_SMALL)).all()) if dt == torch.float32 else torch.equal(got, want)
        assert st.last_indexes.tolist() == [-1] * 4


def test_workspace_reuse_over_changing_shapes():
    """50 consecutive row passes of changing shapes on ONE workspace equal the same calls on fresh
    (zero-filled) workspaces, and leave the reused workspace's arrival counters at zero."""
    from specdec_amd import ops
    g = torch.Generator().manual_seed(12)
    shapes = [(int(torch.randint(1, 9, (1,), generator=g)), [2047, 2048, 4104, 10000, 50257][i % 5],
               [1, 3, 8, 5, 64][(i * 7) % 5], [torch.float32, torch.bfloat16, torch.float16][i % 3]) for i in range(50)]
    rows = [(torch.randn(R, V, generator=g) * 3).to(dt).to(DEV) for R, V, K, dt in shapes]
    ops._WS.clear()
    reused = [ops.beam_topk(x, K) for x, (R, V, K, dt) in zip(rows, shapes)]
    torch.cuda.synchronize()
    (ws,) = ops._WS.values()                      # the one workspace all 50 calls shared
    assert int(ws[:64 * 128].view(torch.int32).abs().sum()) == 0   # counters 0..63 of the common block
    for x, (R, V, K, dt), (lp, tok) in zip(rows, shapes, reused):
        ops._WS.clear()
        lp2, tok2 = ops.beam_topk(x, K)
        assert torch.equal(tok, tok2) and torch.equal(lp, lp2), (R, V, K, dt)


def test_one_workspace_shared_with_verify_sample_and_ngram():
    """beam_step and beam_topk interleaved with ops.verify, sample_rows and ngram_verify on several
    rows, all on ONE workspace, give what the same calls give on fresh zero-filled workspaces: the
    beam partials lie behind the counter block that the other layouts keep at the front, so no call
    finds another's data where its arrival counters are."""
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    V, B, gamma = 128256, 6, 3
    g = torch.Generator().manual_seed(21)
    tl = (torch.randn(B, gamma + 1, V, generator=g) * 3).to(torch.bfloat16).to(DEV)
    dl = (tl[:, :gamma].float() + torch.randn(B, gamma, V, generator=g).to(DEV)).to(torch.bfloat16)
    ids = torch.randint(3, V, (B, gamma), generator=g).to(DEV)
    big = (torch.randn(64, V, generator=g) * 3).to(torch.bfloat16).to(DEV)   # 64 rows x K = 64: > 2 MiB of partials
    stops = torch.tensor([1], dtype=torch.long, device=DEV)
    spec = ops.ProcSpec("multinomial", 1.0)

    def sequence(fresh: bool):
        out = []

        def call(fn):
            if fresh:
                ops._WS.clear()
            out.append(fn())

        def beam():
            st = ops.BeamState.start([5, 9, 2, 81], 4, 12, 0, DEV)
            ops.beam_step(st, big[:1], 4, prefill=True, length=1, stop_tokens=stops)
            ops.beam_step(st, big[:4], 5, top_k=3, length=1, stop_tokens=stops)
            return [st.input_ids.clone(), st.beams_probs.clone(), st.last_indexes.clone()]

        def verify(seed):
            o = ops.verify([tl[:, t] for t in range(gamma + 1)], [dl[:, t] for t in range(gamma)], ids,
                           _lib.SD_RULE_SPEC, spec, spec, PhiloxNoise(seed, 0), stops)
            return [o.n_accepted.clone(), o.next_token.clone(), o.row_status.clone()]

        def sample(seed):
            tok, _, status = ops.sample_rows(tl[:, 0], spec, PhiloxNoise(seed, 0))
            return [tok.clone(), status.clone()]

        def ngram(seed):
            o = ops.ngram_verify([tl[:, t] for t in range(gamma + 1)], ids, spec, PhiloxNoise(seed, 0), stops, filler_k=3)
            return [o.n_accepted.clone(), o.next_token.clone(), o.row_status.clone(), o.filler_ids.clone()]

        call(lambda: verify(1))                    # sizes the shared workspace for everything below
        call(lambda: list(ops.beam_topk(big, 64)))
        call(lambda: verify(2))
        call(beam)
        call(lambda: sample(3))
        call(lambda: list(ops.beam_topk(big[:5], 8)))
        call(lambda: ngram(4))
        call(beam)
        call(lambda: verify(5))
        torch.cuda.synchronize()
        return out

    ops._WS.clear()
    lib = _lib.lib   # the largest layout first, so that no later call replaces the buffer by a bigger, fresh one
    need = max(lib.sd_beam_workspace_size(64, V, 64), lib.sd_verify_workspace_size(B, gamma, V),
               lib.sd_ngram_workspace_size(B, gamma, V), lib.sd_sample_workspace_size(B, V))
    ws = ops._workspace(need, big.device)   # the key the calls use: the tensors' device
    shared = sequence(fresh=False)
    assert len(ops._WS) == 1 and next(iter(ops._WS.values())) is ws
    fresh = sequence(fresh=True)
    for i, (a, b) in enumerate(zip(shared, fresh)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), i
    for o in (shared[0], shared[2], shared[8]):
        assert bool((o[2] & _lib.SD_ROW_DONE).all())   # every sequence's result was written
