"""The vocabulary-parallel verify on the GPU (sd_vp_stats / sd_vp_decide / sd_vp_finish), through the
single-GPU emulation LocalShards unless said otherwise.

* steps against the host model (tests/vocab_parallel_ref.py over the exact-arithmetic oracle and the
  numpy Philox) over vp_cases.grid(), whose coverage tests/test_vocab_parallel_cpu.py proves;
* S = 1 against sd_verify(SD_RULE_SPEC); losslessness on the device; bad layouts; workspace reuse;
  graph capture; two processes on a gloo group; the decode loop with its trace; the torch ops.

A sequence whose host walk had an accept test within the device's fp32 tolerance of its threshold
(`close`) may legitimately differ in its decision; at most one per case does (the CPU test proves the
host model alone stays within that).  owner_shard and next_token are checked without exclusions.
"""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fakelm
import multi_walk as mw
import multidraft_ref as mref
import vocab_parallel_ref as vref
import vp_cases as vc
from oracle import specdec_ref as ref
from test_gpu_perfmode import chi2_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_FIELDS = ("n_accepted", "next_token", "prune_drafter", "prune_target", "stop_index", "row_status", "owner_shard")


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops, vocab_parallel
    from specdec_amd.noise import PhiloxNoise
    return SimpleNamespace(lib=_lib, ops=ops, vp=vocab_parallel, PhiloxNoise=PhiloxNoise)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def bits(out):
    """Every output of one shard as exact integers (resample_mass by its bits)."""
    d = {f: getattr(out, f).cpu() for f in INT_FIELDS}
    d["resample_mass"] = out.resample_mass.cpu().view(torch.int32)
    return d


def run_local(sd, sizes, tl, dl, tok, proc, seed, off, row_base=0, stops=(), skip=False, status_or=None):
    """One LocalShards step on whole rows (sliced as views); asserts every shard returned the same
    bits and returns shard 0's outputs on the host."""
    ls = sd.vp.LocalShards(sd.vp.VocabShard.split(sizes))
    outs = sd.vp.verify_vocab_parallel(tl, dl, tok, spec_of(sd, proc), sd.PhiloxNoise(seed=seed, offset=off), None, ls,
                                       stop_tokens=torch.tensor(list(stops), dtype=torch.long, device=DEV),
                                       row_base=row_base, skip_sample_adjustment=skip, status_or=status_or)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_VP
    assert len(outs) == len(sizes)
    first = bits(outs[0])
    for o in outs[1:]:
        for f, v in bits(o).items():
            assert torch.equal(v, first[f]), f
    got = SimpleNamespace(**first)
    got.mass = outs[0].resample_mass.cpu()
    return got


def mass_tolerance(proc, dtype, t_row, d_row):
    """1e-5 (the project's mass tolerance) plus flip_slack of the target and the drafter row the
    residual was formed from: how far their rounded probabilities can move when the softmax
    normalisers are off by 1e-6."""
    proc_l = lambda x: ref.processed_logits(x, proc, exact=True) / proc.temperature   # noqa: E731
    return 1e-5 + mw.flip_slack(proc_l(t_row), dtype) + mw.flip_slack(proc_l(d_row), dtype)


def check_row(L, tag, r, sizes, stochastic, got_ints, st, x, owner, mass, mass_tol):
    """One sequence against the host model's step r.  Returns False when the decision differs on a
    `close` row (the caller counts those), else True after every check."""
    want = (r.n, r.prune_drafter, r.prune_target, r.stop_index)
    print(f"[vp] {tag} got={got_ints} want={want} close={r.close} status=0x{st:x} x={x} owner={owner} "
          f"mass={mass:.6g}/{r.resample_mass:.6g}")
    assert st & L.SD_ROW_DONE and not st & L.SD_ROW_ERROR_MASK, (tag, hex(st))
    want_bit = {mref.RESIDUAL: L.SD_ROW_RESIDUAL, mref.BONUS: L.SD_ROW_BONUS, mref.STOP: L.SD_ROW_STOP_IN_DRAFTS}[r.status]
    exit_bit = st & (L.SD_ROW_RESIDUAL | L.SD_ROW_BONUS | L.SD_ROW_STOP_IN_DRAFTS | L.SD_ROW_FALLBACK_P)
    if got_ints != want or exit_bit != want_bit:
        assert r.close, (tag, got_ints, want, hex(st))
        return False
    if r.status == mref.RESIDUAL:
        print(f"[vp-mass] {tag} dev={abs(mass - r.resample_mass):.3g} bound={mass_tol():.3g}")
        assert abs(mass - r.resample_mass) <= mass_tol(), (tag, mass, r.resample_mass)
    else:
        assert np.isnan(mass), (tag, mass)
    if r.status == mref.STOP:
        assert x == -1 and owner == -1, (tag, x, owner)
        return True
    w = r.weights
    bs = vref.bounds(sizes)
    assert 0 <= owner < len(bs), (tag, owner)
    o, n = bs[owner]
    assert o <= x < o + n, (tag, x, owner)                  # the token lies in the owner's slice
    if stochastic:
        shard_iv, tok_iv = vref.intervals(w, sizes)
        M, Ms = r.M, r.masses[owner]
        t1, t2 = r.u1 * M, r.u2 * Ms
        print(f"[vp-pick] {tag} u1M={t1:.9g} in [{shard_iv[owner, 0]:.9g}, {shard_iv[owner, 1]:.9g}) "
              f"u2Ms={t2:.9g} in [{tok_iv[x, 0]:.9g}, {tok_iv[x, 1]:.9g}) model owner={r.owner} x={r.x}")
        assert w[x] > 0 and Ms > 0, (tag, x, owner)
        assert shard_iv[owner, 0] - 1e-5 * M <= t1 <= shard_iv[owner, 1] + 1e-5 * M, (tag, owner, r.owner)
        assert tok_iv[x, 0] - 1e-5 * Ms <= t2 <= tok_iv[x, 1] + 1e-5 * Ms, (tag, x, r.x)
    else:
        assert w[x] >= w.max() * (1 - 1e-4), (tag, x, r.x)
        top = np.sort(w)[-2:] if len(w) > 1 else np.array([0.0, w[0]])
        if top[0] < top[1] * (1 - 1e-4):                    # a maximum unique by more than the margin
            assert x == r.x and owner == r.owner, (tag, x, r.x)
    return True


def check_case(sd, c, got, rows):
    close_rows = 0
    for b, r in enumerate(rows):
        ints = (int(got.n_accepted[b]), int(got.prune_drafter[b]), int(got.prune_target[b]), int(got.stop_index[b]))
        tol = lambda: mass_tolerance(c.proc, c.dtype, c.tl[b, r.n], c.dl[b, r.n])   # noqa: E731
        ok = check_row(sd.lib, f"b={b}", r, c.sizes, c.proc.stochastic, ints, int(got.row_status[b]),
                       int(got.next_token[b]), int(got.owner_shard[b]), float(got.mass[b]), tol)
        close_rows += not ok
        if ok and c.dead[b] is not None:
            assert int(got.owner_shard[b]) != c.dead[b]       # a slice of -inf has mass 0: never picked
    print(f"[vp] close rows that differ: {close_rows}")
    assert close_rows <= 1


# ---------------------------------------------------------------- 1. steps against the host model
@pytest.mark.parametrize("case", vc.grid(), ids=vc.case_id)
def test_steps_equal_the_host_model(sd, case):
    c = vc.case(*case)
    rows = vc.host_results(c)
    got = run_local(sd, c.sizes, c.tl.to(DEV), c.dl.to(DEV) if c.gamma else None, c.tok.to(DEV) if c.gamma else None,
                    c.proc, vc.SEED, vc.OFFSET, vc.ROW_BASE, c.stops)
    check_case(sd, c, got, rows)


def test_skip_sample_adjustment_samples_the_target_row(sd):
    case = (16, 4, 4100, (2051, 2048, 1), torch.bfloat16, "multinomial", False, False)
    c = vc.case(*case)
    got = run_local(sd, c.sizes, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, vc.SEED, vc.OFFSET, vc.ROW_BASE,
                    skip=True)
    L, seen = sd.lib, 0
    for b in range(c.B):
        r = vref.step(c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy(), vc.SEED, vc.OFFSET,
                      vc.ROW_BASE + b, c.sizes, skip=True)
        st, x, owner = int(got.row_status[b]), int(got.next_token[b]), int(got.owner_shard[b])
        if r.close or r.status != mref.RESIDUAL:
            continue
        seen += 1
        assert st & L.SD_ROW_FALLBACK_P and not st & L.SD_ROW_RESIDUAL and int(got.n_accepted[b]) == r.n
        assert np.isnan(float(got.mass[b])) and (int(got.prune_drafter[b]), int(got.prune_target[b])) == (4 - r.n, 5 - r.n)
        shard_iv, tok_iv = vref.intervals(r.weights, c.sizes)
        assert shard_iv[owner, 0] - 1e-5 * r.M <= r.u1 * r.M <= shard_iv[owner, 1] + 1e-5 * r.M
        Ms = r.masses[owner]
        assert r.weights[x] > 0 and tok_iv[x, 0] - 1e-5 * Ms <= r.u2 * Ms <= tok_iv[x, 1] + 1e-5 * Ms
    assert seen >= 3


# ---------------------------------------------------------------- 2. S = 1 is sd_verify
@pytest.mark.parametrize("name,V,dtype,stop", [("multinomial", 4096, torch.bfloat16, True),
                                               ("multinomial_T0.7", 1000, torch.float32, False),
                                               ("greedy", 50257, torch.float16, False)])
def test_one_shard_equals_sd_verify(sd, name, V, dtype, stop):
    """Every integer output but next_token (drawn on two uniforms here, another scheme in sd_verify)."""
    c = mw.case(16, 1, 4, V, dtype, name)
    stops = [int(c.tok[3, 0, 0])] if stop else []
    tl, dl, tok = c.tl[:, 0].to(DEV), c.dl[:, 0].to(DEV), c.tok[:, 0].to(DEV)
    got = run_local(sd, (V,), tl, dl, tok, c.proc, mw.SEED, mw.OFFSET, mw.ROW_BASE, stops)
    spec = spec_of(sd, c.proc)
    one = sd.ops.verify([tl[:, t] for t in range(5)], [dl[:, t] for t in range(4)], tok, sd.lib.SD_RULE_SPEC, spec, spec,
                        sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET),
                        torch.tensor(stops, dtype=torch.long, device=DEV), row_base=mw.ROW_BASE)
    for f in ("n_accepted", "prune_drafter", "prune_target", "stop_index", "row_status"):
        assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f
    assert torch.equal(got.owner_shard, torch.where(got.next_token >= 0, 0, -1).int())
    if stop:
        assert int((one.row_status.cpu() & sd.lib.SD_ROW_STOP_IN_DRAFTS != 0).sum()) >= 1


# ---------------------------------------------------------------- 3. losslessness on the device
def test_first_token_and_owner_shard_keep_their_distributions(sd):
    """4096 sequences (row_base 0..4095 in calls of B = 1024) with identical rows, V = 64 over 4 uneven
    shards, γ' = 2, drafts iid from the exact q on the host: the first emitted token against the exact
    target row, and owner_shard of the sequences that left through one exit against M_s / M of that
    exit's weights."""
    V, g, sizes, N, B = 64, 2, (1, 30, 17, 16), 4096, 1024
    gen = torch.Generator().manual_seed(31)
    tl = (torch.randn(g + 1, V, generator=gen) * 2).to(torch.bfloat16)
    dl = (tl[:g].float() + 0.8 * torch.randn(g, V, generator=gen)).to(torch.bfloat16)
    proc = vc.PROCS["multinomial"]
    p = ref.process(tl, proc, exact=True).double().numpy()
    q = ref.process(dl, proc, exact=True).double().numpy()
    rng = np.random.default_rng(77)
    tok = np.stack([rng.choice(V, size=N, p=q[d] / q[d].sum()) for d in range(g)], axis=-1)
    T, D = tl.to(DEV).expand(B, g + 1, V), dl.to(DEV).expand(B, g, V)
    first, owner, n_acc = [], [], []
    for r0 in range(0, N, B):
        got = run_local(sd, sizes, T, D, torch.from_numpy(tok[r0:r0 + B]).to(DEV), proc, 4321, 2, row_base=r0)
        assert int((got.row_status & sd.lib.SD_ROW_ERROR_MASK).abs().sum()) == 0 and int(got.next_token.min()) >= 0
        n = got.n_accepted.numpy()
        first.append(np.where(n >= 1, tok[r0:r0 + B, 0], got.next_token.numpy()))
        owner.append(got.owner_shard.numpy())
        n_acc.append(n)
    first, owner, n_acc = np.concatenate(first), np.concatenate(owner), np.concatenate(n_acc)
    chi2_check(first, p[0], "vocab-parallel first token")
    exits = {0: np.maximum(p[0] - q[0], 0), 1: np.maximum(p[1] - q[1], 0), 2: p[2]}
    checked = 0
    for n, w in exits.items():
        sel = n_acc == n
        if sel.sum() >= 400:
            chi2_check(owner[sel], vref.pick(w, sizes, 0.5, 0.5).masses, f"owner_shard at exit n={n}")
            checked += 1
    assert checked >= 2


# ---------------------------------------------------------------- 4. a bad layout is flagged
def _manual_steps(sd, shards, tl, dl, tok, proc, seed, off, status_or):
    nz, _ = sd.ops._noise_struct(sd.PhiloxNoise(seed=seed, offset=off), 0, tl.device, 0)
    return [sd.vp._step_of(sh.view(tl), sh.view(dl), tok, spec_of(sd, proc), nz, sh, None, False, status_or)
            for sh in shards]


@pytest.mark.parametrize("bad", ["permuted", "short"])
def test_a_bad_layout_is_flagged_not_sampled(sd, bad):
    c = vc.case(5, 4, 37, (1, 35, 1), torch.float16, "multinomial", False, False)
    VS = sd.vp.VocabShard
    shards = VS.split(c.sizes) if bad == "permuted" else [VS(0, 3, 0, 1, 37), VS(1, 3, 1, 30, 37), VS(2, 3, 31, 1, 37)]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    steps = _manual_steps(sd, shards, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, 5, 1, err)
    blocks = [st.stats() for st in steps]
    if bad == "permuted":
        blocks = [blocks[1], blocks[0], blocks[2]]
    stats_all = sd.vp.LocalShards.concat(blocks)
    cand_all = sd.vp.LocalShards.concat([st.decide(stats_all) for st in steps])
    for st in steps:
        out = st.finish(cand_all)
        assert torch.equal(out.row_status.cpu(), torch.full((5,), sd.lib.SD_ROW_DONE | sd.lib.SD_ROW_INVALID_DIST,
                                                            dtype=torch.int32))
        assert int(out.next_token.max()) == -1 and int(out.owner_shard.max()) == -1
        assert int(out.n_accepted.abs().sum()) == 0
    assert int(err.item()) == sd.lib.SD_ROW_INVALID_DIST


def test_a_wrong_exchange_shape_is_a_value_error(sd):
    c = vc.case(5, 4, 37, (1, 35, 1), torch.float16, "multinomial", False, False)
    sh = sd.vp.VocabShard.split(c.sizes)[1]
    with pytest.raises(ValueError):
        sd.vp.verify_vocab_parallel(sh.view(c.tl.to(DEV)), sh.view(c.dl.to(DEV)), c.tok.to(DEV), spec_of(sd, c.proc),
                                    sd.PhiloxNoise(seed=1), sh, lambda blk: torch.stack([blk, blk]))


# ---------------------------------------------------------------- 5. workspace reuse
def test_one_workspace_serves_every_entry_point_in_turn(sd):
    c = vc.case(16, 4, 4100, (2051, 2048, 1), torch.bfloat16, "multinomial", False, False)
    tl, dl, tok = c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV)
    spec = spec_of(sd, c.proc)
    m = mw.case(3, 2, 4, 4096, torch.bfloat16, "multinomial")

    def vp():
        return run_local(sd, c.sizes, tl, dl, tok, c.proc, 99, 4, 2)

    def others():
        sd.ops.verify([tl[:, t] for t in range(5)], [dl[:, t] for t in range(4)], tok, sd.lib.SD_RULE_SPEC, spec, spec,
                      sd.PhiloxNoise(seed=1))
        sd.ops.sample_rows(tl[:, 0].contiguous(), spec, sd.PhiloxNoise(seed=2))
        return sd.ops.verify_multi(m.tl.to(DEV), m.dl.to(DEV), m.tok.to(DEV), spec, sd.PhiloxNoise(seed=3, offset=1))

    sd.ops._WS.clear()
    fresh_vp = vp()
    sd.ops._WS.clear()
    fresh_multi = others()
    sd.ops._WS.clear()
    a = vp()
    multi = others()
    b = vp()
    for got in (a, b):
        for f in INT_FIELDS + ("resample_mass",):
            assert torch.equal(getattr(got, f), getattr(fresh_vp, f)), f
    for f in sd.ops.MULTI_FIELDS:
        assert torch.equal(getattr(multi, f).cpu().view(torch.int32), getattr(fresh_multi, f).cpu().view(torch.int32)), f


# ---------------------------------------------------------------- 6. graph capture
def test_a_step_is_capturable_and_replays_with_fresh_noise(sd):
    c = vc.case(5, 4, 4100, (2051, 2048, 1), torch.float32, "multinomial_T0.7", False, False)
    tl, dl, tok = c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV)
    ls = sd.vp.LocalShards(sd.vp.VocabShard.split(c.sizes))
    spec = spec_of(sd, c.proc)
    eager = [run_local(sd, c.sizes, tl, dl, tok, c.proc, 808, 5 + k, 1) for k in range(3)]
    od = torch.zeros(1, dtype=torch.long, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = sd.vp.verify_vocab_parallel(tl, dl, tok, spec, sd.PhiloxNoise(seed=808, offset=5, offset_dev=od), None, ls,
                                           row_base=1)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for o in outs:
            for f, v in bits(o).items():
                assert torch.equal(v, getattr(eager[k], f)), (k, f)
        od.add_(1)                                        # the offset advances on the device


# ---------------------------------------------------------------- 7. two processes
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


TWO = (5, 4, 4100, (2051, 2049), torch.bfloat16, "multinomial", False, True)


def _rank_worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        torch.cuda.set_device(0)
        from specdec_amd import ops, vocab_parallel as vp
        from specdec_amd.noise import PhiloxNoise
        c = vc.case(*TWO)
        sh = vp.VocabShard.split(c.sizes)[rank]
        o = vp.verify_vocab_parallel(sh.view(c.tl.to(DEV)), sh.view(c.dl.to(DEV)), c.tok.to(DEV),
                                     ops.ProcSpec(c.proc.kind, c.proc.temperature), PhiloxNoise(seed=vc.SEED, offset=vc.OFFSET),
                                     sh, vp.GroupExchange(dist.group.WORLD),
                                     stop_tokens=torch.tensor(list(c.stops), dtype=torch.long, device=DEV),
                                     row_base=vc.ROW_BASE)
        out.put((rank, {f: v.tolist() for f, v in bits(o).items()}))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_a_gloo_group_equal_the_emulation(sd):
    c = vc.case(*TWO)
    want = run_local(sd, c.sizes, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, vc.SEED, vc.OFFSET, vc.ROW_BASE,
                     c.stops)
    check_case(sd, c, want, vc.host_results(c))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in (0, 1):
        for f in INT_FIELDS + ("resample_mass",):
            assert got[rank][f] == getattr(want, f).tolist(), (rank, f)


# ---------------------------------------------------------------- 8. the loop
@pytest.mark.parametrize("name", ["greedy", "multinomial"])
def test_loop_steps_replay_through_the_host_model(sd, name):
    from specdec_amd.sampling import vocab_parallel_speculative_generate
    from specdec_amd.utils.logits_processor import GreedyProcessor, MultinomialProcessor
    V, g, S = 4096, 4, 4
    target, drafter = fakelm.make_pair(V, sigma=1.0, device=DEV)
    ls = sd.vp.LocalShards.even(S, V)
    sizes = [sh.vocab_local for sh in ls.shards]
    fns = [(lambda ids, sh=sh: sh.view(target(input_ids=ids).logits)) for sh in ls.shards]
    proc = GreedyProcessor() if name == "greedy" else MultinomialProcessor(1.0)
    rproc = vc.PROCS[name]
    prompt, seed, trace = [3, 17, 5, 9], 2024, []
    toks, rate = vocab_parallel_speculative_generate(prompt, drafter, fns, None, ls, gamma=g, logits_processor=proc,
                                                     max_gen_len=48, eos_tokens_id=-1, seed=seed, trace=trace)
    assert len(toks) == 48 and min(toks) >= 0
    cur, seq, close_rows, acc, spec_n = len(prompt), list(prompt), 0, 0, 0
    for i, (off, drafts, n, x, status) in enumerate(trace):
        gp = len(drafts)
        tok = np.array(drafts, dtype=np.int64).reshape(1, gp)
        if gp:
            P, Q = mw.step_rows(target, drafter, seq[-1], cur, tok, rproc)
        else:                                               # the first-target token: one target row, no drafts
            P, Q = mw.bank_rows(target, [seq[-1]], [cur - 1], rproc)[None], np.zeros((1, 0, V))
        r = vref.step(P[0], Q[0], tok[0], seed, off, 0, sizes, (-1,), greedy=name == "greedy")
        pruned = (gp - n, gp - n + 1) if (n < gp and not status & sd.lib.SD_ROW_STOP_IN_DRAFTS) else (0, 0)
        owner = next(s for s, (o, m) in enumerate(vref.bounds(sizes)) if o <= x < o + m)
        ok = check_row(sd.lib, f"step={i}", r, sizes, rproc.stochastic, (n, *pruned, -1), status, x, owner,
                       r.resample_mass, lambda: 0.0)        # the loop reads neither the mass nor the owner back
        close_rows += not ok
        assert toks[cur - len(prompt):cur - len(prompt) + n] == drafts[:n] and toks[cur - len(prompt) + n] == x
        seq += drafts[:n] + [x]
        cur += n + 1
        acc, spec_n = acc + n, spec_n + gp
    assert close_rows <= 1
    assert seq[len(prompt):] == toks and rate == pytest.approx(acc / spec_n) and 0 < rate < 1


def test_loop_stops_on_an_eos_token(sd):
    from specdec_amd.sampling import vocab_parallel_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor, TopKProcessor
    V = 4096
    target, drafter = fakelm.make_pair(V, sigma=1.0, device=DEV)
    ls = sd.vp.LocalShards.even(4, V)
    fns = [(lambda ids, sh=sh: sh.view(target(input_ids=ids).logits)) for sh in ls.shards]
    eos = fakelm.likely_tokens(target)
    toks, _ = vocab_parallel_speculative_generate([3, 17, 5, 9], drafter, fns, None, ls, gamma=4,
                                                  logits_processor=MultinomialProcessor(1.0), max_gen_len=48,
                                                  eos_tokens_id=eos, seed=7)
    assert toks[-1] in eos and not set(toks[:-1]) & set(eos) and len(toks) < 48
    with pytest.raises(TypeError):
        vocab_parallel_speculative_generate([3], drafter, fns, None, ls, logits_processor=TopKProcessor(1.0, 50))


# ---------------------------------------------------------------- 9. the torch ops
def test_torch_ops_equal_the_python_entry_point(sd):
    c = vc.case(5, 4, 4100, (2051, 2048, 1), torch.float32, "multinomial_T0.7", False, False)
    tl, dl, tok = c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV)
    want = run_local(sd, c.sizes, tl, dl, tok, c.proc, 606, 3, 2)
    shards = sd.vp.VocabShard.split(c.sizes)
    stops = torch.empty(0, dtype=torch.long, device=DEV)
    kind, T = sd.lib.SD_PROC_MULTINOMIAL, 0.7
    op = torch.ops.specdec
    stats = torch.stack([op.vp_stats(sh.view(tl), sh.view(dl), tok, sh.shard, 3, sh.vocab_offset, c.V, kind, T)
                         for sh in shards])
    cand = torch.stack([op.vp_decide(sh.view(tl), sh.view(dl), tok, stops, stats, sh.shard, 3, sh.vocab_offset, c.V, kind,
                                     T, False, 606, 3, 2) for sh in shards])
    for sh in shards:
        out = op.vp_finish(cand, 4, sh.shard, 3, sh.vocab_offset, sh.vocab_local, c.V, kind, 606, 3, 2)
        for f, v in zip(sd.vp.VP_FIELDS, out):
            assert torch.equal(v.cpu().view(torch.int32) if f == "resample_mass" else v.cpu(), getattr(want, f)), f
    assert stats.shape == (3, 32 + 5 * 9 * 16) and cand.shape == (3, 32 + 5 * 32) and stats.dtype == torch.uint8
    m = torch.empty(5, 5, 100, device="meta"), torch.empty(5, 4, 100, device="meta"), torch.empty(5, 4, dtype=torch.long, device="meta")
    assert op.vp_stats(*m, 0, 2, 0, 200, kind, T).shape == (32 + 5 * 9 * 16,)
