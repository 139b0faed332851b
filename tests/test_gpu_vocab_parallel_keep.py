"""The vocabulary-parallel verify under top-k / nucleus processors (sd_vp_keep_*) on the GPU, through
LocalShards, against the oracle's keep rule on the WHOLE rows
(ref.processed_logits(row, Processor(..., stable_ties=True), exact=True)):

* every output equals verify_vocab_parallel (multinomial, same temperature and noise) on the
  oracle-masked rows, resample_mass within test_gpu_vocab_parallel.mass_tolerance; n, the prune lengths
  and the stop index equal the host model (tests/vocab_parallel_ref.py) on the oracle's probabilities;
* the kept set of EVERY row: each row sampled as a γ' = 0 step through the torch ops, whose candidate
  blocks carry the mass of the kept set inside each slice, against the oracle's probabilities summed over
  that slice (exactly 0 where the oracle drops the whole slice), and the oracle's kept set against the
  support of ops.probs_rows where no kept probability is near the dtype's underflow (asserted);
* nucleus margins are a condition of the case: the fp64 cumulative mass on both sides of every cut is
  asserted to lie more than 1e-4 from top_p (and from the 16-bit rounding boundary above round_dt(top_p),
  where the rule's comparison of the rounded cumulative sum flips), and no row is SD_ROW_NUCLEUS_INEXACT;
* constructed rows; S = 1 equals sd_verify; graph capture; a permuted block A; the torch ops; the loop;
  fp32 rows and STREAM noise are refused.
"""
import ctypes as C
from types import SimpleNamespace
from unittest import mock

import numpy as np
from types import SimpleNamespace

import pytest
import torch

import fakelm
import multi_walk as mw
import multidraft_ref as mref
import vocab_parallel_ref as vref
from oracle import specdec_ref as ref
from test_gpu_vocab_parallel import INT_FIELDS, mass_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = {4100: (2051, 2048, 1), 300: (7, 1, 292)}
PROCS = {"topk1": ("topk", 1, 1.0), "topk50": ("topk", 50, 1.0), "topkV": ("topk", 5000, 1.0),
         "nuc1e-6": ("nucleus", 0, 1e-6), "nuc0.5": ("nucleus", 0, 0.5), "nuc0.9": ("nucleus", 0, 0.9),
         "topk50nuc0.9": ("topknucleus", 50, 0.9), "topk2000nuc0.5": ("topknucleus", 2000, 0.5)}
# (V, B, γ', dtype, temperature); the seed of every (shape, processor) is the first whose rows meet the margins
SHAPES = [(4100, 5, 4, torch.bfloat16, 1.0), (4100, 1, 1, torch.float16, 0.7), (300, 5, 0, torch.float16, 1.0),
          (300, 1, 4, torch.bfloat16, 0.7), (300, 5, 1, torch.bfloat16, 1.0)]
SEEDS = {}   # filled below: (shape index, processor name) -> seed


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops, vocab_parallel
    from specdec_amd.noise import PhiloxNoise, StreamNoise
    return SimpleNamespace(lib=_lib, ops=ops, vp=vocab_parallel, PhiloxNoise=PhiloxNoise, StreamNoise=StreamNoise)


def oracle_proc(name, T):
    kind, k, p = PROCS[name]
    return ref.Processor(kind, T, k, p, stable_ties=True)


def oracle_masked(x, proc):
    """ref.processed_logits(x, proc, exact=True).  The oracle's fill (-1e20) does not fit fp16, where its
    masked_fill raises: there the oracle's own code runs with -inf as the fill (probability 0 either way)."""
    with mock.patch.object(ref, "NEG_FILL", float("-inf") if x.dtype == torch.float16 else ref.NEG_FILL):
        return ref.processed_logits(x, proc, exact=True)


def make_rows(V, B, g, dtype, proc, seed):
    """Peaked rows (the probability at a nucleus cut is well above the margin), drafts drawn from the
    oracle's q so that tests accept and reject."""
    gen = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, g + 1, V, generator=gen) * 8).to(dtype)
    dl = (tl[:, :g].float() + 2 * torch.randn(B, g, V, generator=gen)).to(dtype)
    tok = torch.zeros(B, max(g, 1), dtype=torch.long)
    for b in range(B):
        for d in range(g):
            tok[b, d] = torch.multinomial(ref.softmax(oracle_masked(dl[b, d], proc) / proc.temperature, True).float(), 1,
                                          generator=gen)
    return tl, dl, tok


def margins_ok(rows, proc):
    """The fp64 cumulative mass (of the dtype-rounded probabilities, descending) on both sides of every
    row's cut is more than 1e-4 from top_p and from the rounding boundary above round_dt(top_p)."""
    if proc.kind not in ("nucleus", "topknucleus"):
        return True
    tpd = torch.tensor(proc.top_p).to(rows.dtype)
    up = torch.nextafter(tpd.float(), torch.tensor(2.0)) if rows.dtype == torch.float32 else \
        (tpd.view(torch.int16) + 1).view(rows.dtype)
    marks = (proc.top_p, (tpd.double().item() + up.double().item()) / 2)
    for row in rows.reshape(-1, rows.shape[-1]):
        x = oracle_masked(row, ref.Processor("topk", 1.0, proc.top_k)) if proc.kind == "topknucleus" else row
        p = ref.softmax(x, exact=True).double().sort(descending=True).values.cumsum(0)
        kept = int((oracle_masked(row, proc).float() > -1e19).sum())
        sides = [p[kept - 1].item()] + ([p[kept - 2].item()] if kept > 1 else [])
        if any(abs(c - m) <= 1e-4 for c in sides for m in marks):
            return False
        # the rule's own exactness conditions (SD_ROW_NUCLEUS_INEXACT): the cut's p >= 2^-17, the sum below 1
        if kept < len(p) and (sides[0] >= 1.0 or sides[0] - (sides[1] if kept > 1 else 0.0) < 2.0 ** -17):
            return False
    return True


def case_rows(i, name):
    V, B, g, dtype, T = SHAPES[i]
    proc = oracle_proc(name, T)
    tl, dl, tok = make_rows(V, B, g, dtype, proc, SEEDS[(i, name)])
    return V, B, g, dtype, proc, tl, dl, tok


def run_keep(sd, sizes, tl, dl, tok, proc, noise, keep=True, **kw):
    """One LocalShards step; every shard must return the same bits; shard 0's outputs on the host."""
    ls = sd.vp.LocalShards(sd.vp.VocabShard.split(sizes))
    g = tl.shape[1] - 1
    spec = sd.ops.ProcSpec(proc.kind, proc.temperature, proc.top_k, proc.top_p)
    fn = sd.vp.verify_vocab_parallel_keep if keep else sd.vp.verify_vocab_parallel
    outs = fn(tl.to(DEV), dl.to(DEV) if g else None, tok.to(DEV) if g else None, spec, noise, None, ls, **kw)
    torch.cuda.synchronize()
    for o in outs[1:]:
        for f in INT_FIELDS:
            assert torch.equal(getattr(o, f), getattr(outs[0], f)), f
        assert torch.equal(o.resample_mass.view(torch.int32), outs[0].resample_mass.view(torch.int32))
    return SimpleNamespace(**{f: getattr(outs[0], f).cpu() for f in INT_FIELDS + ("resample_mass",)})


def check_against_masked(sd, sizes, tl, dl, tok, proc, dtype, seed=11, off=3):
    """The keep step on the raw rows == the multinomial step on the oracle-masked rows."""
    mt, md = oracle_masked(tl, proc), oracle_masked(dl, proc)
    plain = ref.Processor("multinomial", proc.temperature)
    got = run_keep(sd, sizes, tl, dl, tok, proc, sd.PhiloxNoise(seed=seed, offset=off), row_base=5)
    want = run_keep(sd, sizes, mt, md, tok, plain, sd.PhiloxNoise(seed=seed, offset=off), keep=False, row_base=5)
    assert not (got.row_status & (sd.lib.SD_ROW_NUCLEUS_INEXACT | sd.lib.SD_ROW_ERROR_MASK)).any()
    for f in INT_FIELDS:
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    for b in range(tl.shape[0]):
        n = int(got.n_accepted[b])
        if int(got.row_status[b]) & sd.lib.SD_ROW_RESIDUAL:
            tol = mass_tolerance(plain, dtype, mt[b, n], md[b, n])
            assert abs(float(got.resample_mass[b]) - float(want.resample_mass[b])) <= tol, (b, tol)
        else:
            assert torch.isnan(got.resample_mass[b])
    # the host model on the oracle's probabilities of the whole rows; a test within the device's fp32
    # tolerance of its threshold (`close`) may differ, in at most one sequence (as test_gpu_vocab_parallel)
    g, T, differ = tl.shape[1] - 1, proc.temperature, 0
    P, Q = (ref.softmax(m / T, exact=True).double().numpy() for m in (mt, md))
    for b in range(tl.shape[0]):
        r = vref.step(P[b], Q[b] if g else np.zeros((0, P.shape[-1])), tok[b, :g].numpy(), seed, off, 5 + b, sizes)
        ints = tuple(int(getattr(got, f)[b]) for f in ("n_accepted", "prune_drafter", "prune_target", "stop_index"))
        if ints != (r.n, r.prune_drafter, r.prune_target, r.stop_index):
            assert r.close, (b, ints, r.n)
            differ += 1
    assert differ <= 1
    return got


def op_args(sd, sh, V, proc):
    return (sh.shard, sh.num_shards, sh.vocab_offset, V, sd.ops.KIND[proc.kind], proc.temperature, proc.top_k, proc.top_p)


def op_step(sd, sizes, tl, dl, tok, proc, seed, off, row_base, permute=False):
    """One step through torch.ops.specdec.vp_keep_*: (the outputs of every shard, the candidate blocks)."""
    op, V, shards = torch.ops.specdec, tl.shape[-1], sd.vp.VocabShard.split(sizes)
    stops = torch.empty(0, dtype=torch.long, device=DEV)
    sl = [(sh.view(tl), sh.view(dl), tok) for sh in shards]
    hist = torch.stack([op.vp_keep_hist(*x, *op_args(sd, sh, V, proc)) for x, sh in zip(sl, shards)])
    if permute:
        hist = hist[[1, 0] + list(range(2, len(shards)))].contiguous()
    bins = []
    for _ in range(sd.lib.lib.sd_vp_keep_rounds(sd.ops.KIND[proc.kind])):
        bins.append(torch.stack([op.vp_keep_refine(*x, hist, bins, *op_args(sd, sh, V, proc)) for x, sh in zip(sl, shards)]))
    cand = torch.stack([op.vp_keep_decide(*x, stops, hist, bins, *op_args(sd, sh, V, proc), False, seed, off, row_base)
                        for x, sh in zip(sl, shards)])
    outs = [op.vp_keep_finish(cand, tl.shape[1] - 1, sh.shard, len(shards), sh.vocab_offset, sh.vocab_local, V,
                              sd.ops.KIND[proc.kind], proc.top_k, proc.top_p, seed, off, row_base) for sh in shards]
    return outs, cand


CASES = [(i, name) for i in range(len(SHAPES)) for name in PROCS]
SEEDS.update(zip(CASES, [   # one row per shape
    0, 0, 0, 1, 1, 5, 5, 1,
    0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 3, 3, 3, 3, 3,
    0, 0, 0, 1, 1, 1, 1, 1,
]))


@pytest.mark.parametrize("i,name", CASES, ids=[f"s{i}-{n}" for i, n in CASES])
def test_keep_step_equals_the_oracle_masked_step(sd, i, name):
    V, B, g, dtype, proc, tl, dl, tok = case_rows(i, name)
    assert margins_ok(tl, proc) and margins_ok(dl, proc)
    check_against_masked(sd, SIZES[V], tl, dl, tok, proc, dtype)
    # the oracle's kept set is the support of the library's whole-row probabilities
    spec = sd.ops.ProcSpec(proc.kind, proc.temperature, proc.top_k, proc.top_p)
    rows = tl.reshape(-1, V)
    masked = torch.cat([oracle_masked(tl, proc).reshape(-1, V), oracle_masked(dl, proc).reshape(-1, V)])
    rows = torch.cat([rows, dl.reshape(-1, V)])
    kept, P = masked.float() > -1e19, ref.softmax(masked / proc.temperature, exact=True).double()
    # every row's kept set in the sharded step: the row as a γ' = 0 sequence; its candidate records carry
    # M_s = Σ of the kept probabilities inside slice s
    dev_rows = rows.to(DEV).unsqueeze(1)
    _, cand = op_step(sd, SIZES[V], dev_rows, dev_rows[:, :0], torch.zeros(len(rows), 1, dtype=torch.long, device=DEV),
                      proc, 11, 3, 0)
    R = len(rows)
    for s, (o, n) in enumerate(vref.bounds(SIZES[V])):
        recs = (sd.lib.sd_vp_cand * R).from_buffer_copy(cand[s, 32:].cpu().numpy().tobytes())
        for r in range(R):
            want = float(P[r, o:o + n].sum())
            tol = 1e-5 + mw.flip_slack(masked[r] / proc.temperature, dtype)
            assert abs(recs[r].mass - want) <= tol, (r, s, recs[r].mass, want)
            assert kept[r, o:o + n].any() or recs[r].mass == 0.0, (r, s)     # a dropped slice: exactly 0
    # the whole-row library keeps the same set: equality of the supports, where no kept probability is
    # within a factor 4 of the dtype's smallest subnormal (a condition of the comparison, asserted where it
    # holds for the whole row; rows with deeper tails are compared above that level)
    tiny = 4 * torch.finfo(dtype).smallest_normal * 2.0 ** -(10 if dtype == torch.float16 else 7)
    support = sd.ops.probs_rows(rows.to(DEV), spec).cpu() > 0
    clear = ~(kept & (P < tiny)).any(-1)
    assert torch.equal(support[clear], kept[clear])
    assert not (support & ~kept).any() and support[kept & (P >= tiny)].all()


def edge_rows(kind):
    """B = 1, γ' = 1, V = 300 over (7, 1, 292), bf16: (target rows [1, 2, V], drafter rows [1, 1, V], tok, processor)."""
    V = 300
    t = torch.full((1, 2, V), -4.0)
    d = torch.full((1, 1, V), -4.0)
    tok = torch.tensor([[2]])
    proc = ref.Processor("nucleus", 1.0, 0, 0.7, stable_ties=True)
    if kind == "tie_across_border":
        # 12 equal values from index 2 (five in shard 0, shard 1's one element, six in shard 2), 9 kept: the run
        # straddles both borders and the quota ends inside the last shard's six (the partial-quota scan); with
        # "tie_ends_in_second" below the quota ends inside the second shard of a two-way split
        t[:, :, 2:14] = 3.0
        d[:, :, 2:14] = 3.0
    elif kind == "negative_cut":         # the max positive, the cut among negative values
        t[:, :, :] = -9.0
        t[:, :, 5] = 0.5
        t[:, :, 20:60] = -1.0
        d.copy_(t[:, :1])
        tok[0, 0] = 25
    elif kind == "all_equal":
        t[:, :, :] = 1.5
        d[:, :, :] = 1.5
    elif kind == "neg_inf":
        t[:, :, 2:14] = 3.0
        t[:, :, 100:200] = float("-inf")
        d.copy_(t[:, :1])
    elif kind == "shard_dropped":        # everything kept lies in shard 2: shards 0 and 1 have M_s = 0
        t[:, :, 50:60] = 5.0
        d.copy_(t[:, :1])
        tok[0, 0] = 52
    elif kind == "target_drops_draft":   # the drafter keeps id 2, the target's keep drops it: reject
        t[:, :, 50:60] = 5.0
        d[:, :, 2] = 6.0
    elif kind == "drafter_drops_draft":  # the drafter's keep drops id 2 (q = 0): accept
        t[:, :, 2] = 6.0
        d[:, :, 50:60] = 5.0
    return t.to(torch.bfloat16), d.to(torch.bfloat16), tok, proc


@pytest.mark.parametrize("kind", ["tie_across_border", "negative_cut", "all_equal", "neg_inf", "shard_dropped",
                                  "target_drops_draft", "drafter_drops_draft"])
def test_constructed_rows(sd, kind):
    tl, dl, tok, proc = edge_rows(kind)
    assert margins_ok(tl, proc) and margins_ok(dl, proc)
    got = check_against_masked(sd, SIZES[300], tl, dl, tok, proc, torch.bfloat16)
    if kind == "target_drops_draft":
        assert int(got.n_accepted[0]) == 0
    if kind == "drafter_drops_draft":
        assert int(got.n_accepted[0]) == 1
    if kind == "shard_dropped":
        assert int(got.owner_shard[0]) == 2


def test_one_shard_equals_sd_verify(sd):
    V, B, g, dtype = 4096, 5, 4, torch.bfloat16
    proc = ref.Processor("nucleus", 1.0, 0, 0.9, stable_ties=True)
    tl, dl, tok = make_rows(V, B, g, dtype, proc, 1)
    assert margins_ok(tl, proc) and margins_ok(dl, proc)
    got = run_keep(sd, (V,), tl, dl, tok, proc, sd.PhiloxNoise(seed=11, offset=3), row_base=5)
    spec = sd.ops.ProcSpec("nucleus", 1.0, 0, 0.9)
    tld, dld = tl.to(DEV), dl.to(DEV)
    one = sd.ops.verify([tld[:, t] for t in range(g + 1)], [dld[:, t] for t in range(g)], tok.to(DEV),
                        sd.lib.SD_RULE_SPEC, spec, spec, sd.PhiloxNoise(seed=11, offset=3), row_base=5)
    for f in ("n_accepted", "prune_drafter", "prune_target", "stop_index", "row_status"):
        assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f


def test_fp32_rows_and_stream_noise_are_refused(sd):
    V = 300
    proc = ref.Processor("nucleus", 1.0, 0, 0.9)
    tl, dl, tok = make_rows(V, 1, 1, torch.float32, proc, 0)
    with pytest.raises(Exception, match="(?i)unsupported"):
        run_keep(sd, SIZES[V], tl, dl, tok, proc, sd.PhiloxNoise(seed=1, offset=0))
    with pytest.raises(TypeError, match="PhiloxNoise"):
        run_keep(sd, SIZES[V], tl.bfloat16(), dl.bfloat16(), tok, proc, sd.StreamNoise(torch.Generator().manual_seed(0)))
    with pytest.raises(TypeError, match="top-k, nucleus"):
        run_keep(sd, SIZES[V], tl.bfloat16(), dl.bfloat16(), tok, ref.Processor("multinomial", 1.0),
                 sd.PhiloxNoise(seed=1, offset=0))


def test_a_tie_quota_ending_inside_the_second_shard(sd):
    """V = 300 over (7, 293): 12 equal values from index 2, nine kept: five in shard 0, four of shard 1's seven."""
    tl, dl, tok, proc = edge_rows("tie_across_border")
    got = check_against_masked(sd, (7, 293), tl, dl, tok, proc, torch.bfloat16)
    assert int(got.row_status[0]) & sd.lib.SD_ROW_DONE


def test_a_cut_in_another_high_byte_bin_than_the_max(sd):
    """A bf16 key's high byte holds two octaves: the max 9.0 lies in [8, 32), the cut inside the run of forty 3.0
    in [2, 8), and the dropped 1.0 in [0.5, 2): the crossing bin is neither the max's nor the lowest."""
    V = 300
    t = torch.full((1, 2, V), 1.0)
    t[:, :, 9] = 9.0
    t[:, :, 100:140] = 3.0
    proc = ref.Processor("nucleus", 1.0, 0, 0.9, stable_ties=True)
    tl = t.to(torch.bfloat16)
    dl, tok = tl[:, :1].clone(), torch.tensor([[105]])
    assert margins_ok(tl, proc)
    kept = oracle_masked(tl[0, 0], proc).float() > -1e19
    assert kept[9] and 1 < int(kept.sum()) < 41 and not kept[0]        # the cut lies inside the run of 3.0
    check_against_masked(sd, SIZES[V], tl, dl, tok, proc, torch.bfloat16)


def test_a_step_is_capturable_and_replays_with_fresh_noise(sd):
    V, B, g, dtype, proc, tl, dl, tok = case_rows(0, "nuc0.9")
    tl, dl, tok = tl.to(DEV), dl.to(DEV), tok.to(DEV)
    ls = sd.vp.LocalShards(sd.vp.VocabShard.split(SIZES[V]))
    spec = sd.ops.ProcSpec(proc.kind, proc.temperature, proc.top_k, proc.top_p)
    eager = [run_keep(sd, SIZES[V], tl, dl, tok, proc, sd.PhiloxNoise(seed=808, offset=5 + k), row_base=1) for k in range(3)]
    od = torch.zeros(1, dtype=torch.long, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = sd.vp.verify_vocab_parallel_keep(tl, dl, tok, spec, sd.PhiloxNoise(seed=808, offset=5, offset_dev=od), None,
                                                ls, row_base=1)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for o in outs:
            for f in INT_FIELDS:
                assert torch.equal(getattr(o, f).cpu(), getattr(eager[k], f)), (k, f)
            assert torch.equal(o.resample_mass.cpu().view(torch.int32), eager[k].resample_mass.view(torch.int32)), k
        od.add_(1)


def test_torch_ops_equal_the_python_entry_point_and_a_permuted_block_flags_every_row(sd):
    V, B, g, dtype, proc, tl, dl, tok = case_rows(0, "topk50nuc0.9")
    want = run_keep(sd, SIZES[V], tl, dl, tok, proc, sd.PhiloxNoise(seed=606, offset=3), row_base=2)
    outs, cand = op_step(sd, SIZES[V], tl.to(DEV), dl.to(DEV), tok.to(DEV), proc, 606, 3, 2)
    for out in outs:
        for f, v in zip(sd.vp.VP_FIELDS, out):
            assert torch.equal(v.cpu().view(torch.int32), getattr(want, f).view(torch.int32)), f
    assert cand.shape == (3, 32 + B * 32) and cand.dtype == torch.uint8
    outs, _ = op_step(sd, SIZES[V], tl.to(DEV), dl.to(DEV), tok.to(DEV), proc, 606, 3, 2, permute=True)
    for out in outs:
        o = dict(zip(sd.vp.VP_FIELDS, out))
        assert torch.equal(o["row_status"].cpu(), torch.full((B,), sd.lib.SD_ROW_DONE | sd.lib.SD_ROW_INVALID_DIST,
                                                             dtype=torch.int32))
        assert int(o["next_token"].max()) == -1 and int(o["owner_shard"].max()) == -1 and int(o["n_accepted"].abs().sum()) == 0


def test_loop_steps_replay_through_the_host_model(sd):
    from specdec_amd.sampling import vocab_parallel_speculative_generate
    from specdec_amd.utils.logits_processor import NucleusProcessor
    V, g, S = 4096, 4, 4
    target, drafter = fakelm.make_pair(V, sigma=1.0, device=DEV)
    ls = sd.vp.LocalShards.even(S, V)
    sizes = [sh.vocab_local for sh in ls.shards]
    fns = [(lambda ids, sh=sh: sh.view(target(input_ids=ids).logits)) for sh in ls.shards]
    rproc = ref.Processor("nucleus", 1.0, 0, 0.9, stable_ties=True)
    prompt, seed, trace = [3, 17, 5, 9], 2024, []
    with pytest.raises(TypeError):
        vocab_parallel_speculative_generate(prompt, drafter, fns, None, ls, logits_processor=NucleusProcessor(1.0, 0.9))
    toks, rate = vocab_parallel_speculative_generate(prompt, drafter, fns, None, ls, gamma=g,
                                                     logits_processor=NucleusProcessor(1.0, 0.9), max_gen_len=32,
                                                     eos_tokens_id=-1, seed=seed, trace=trace, sharded_keep=True)
    assert len(toks) == 32 and min(toks) >= 0
    cur, seq, differ, acc, spec_n = len(prompt), list(prompt), 0, 0, 0
    for off, drafts, n, x, status in trace:
        gp = len(drafts)
        tok = np.array(drafts, dtype=np.int64).reshape(1, gp)
        if gp:
            P, Q = mw.step_rows(target, drafter, seq[-1], cur, tok, rproc)
        else:
            P, Q = mw.bank_rows(target, [seq[-1]], [cur - 1], rproc)[None], np.zeros((1, 0, V))
        r = vref.step(P[0], Q[0], tok[0], seed, off, 0, sizes, (-1,))
        assert not status & (sd.lib.SD_ROW_ERROR_MASK | sd.lib.SD_ROW_NUCLEUS_INEXACT)
        if n != r.n:
            assert r.close
            differ += 1
        elif r.status != mref.STOP:
            assert r.weights[x] > 0                       # the emitted token lies in the oracle's residual support
        seq += drafts[:n] + [x]
        cur += n + 1
        acc, spec_n = acc + n, spec_n + gp
    assert differ <= 1 and seq[len(prompt):] == toks and rate == pytest.approx(acc / spec_n) and 0 < rate < 1
