"""CPU checks of the vocabulary-parallel verify: the ctypes mirrors against the header, the rule's
exactness by enumeration over (u1, u2), the host model's independence from the sharding, the coverage
of the GPU case grid (tests/test_gpu_vocab_parallel.py runs exactly vp_cases.grid()) and the exchange
plumbing on two gloo ranks."""
import ctypes as C
import os
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import multidraft_ref as mref
import vocab_parallel_ref as vref
import vp_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- struct layout
def test_vp_structs_ctypes_layout_matches_the_header():
    """sizeof and field offsets of sd_vp_args and the exchanged records: the ctypes mirrors against the
    C header (gcc); the ABI number and every existing struct's size stay."""
    from specdec_amd import _lib
    structs = ["sd_vp_args", "sd_vp_header", "sd_vp_stat", "sd_vp_cand"]
    old = ["sd_verify_args", "sd_sample_args", "sd_ngram_args", "sd_beam_args", "sd_multi_args"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
    for s in structs:
        prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
        for f, _ in getattr(_lib, s)._fields_:
            prog += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    for s in old:
        prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
    prog += ('  printf("limits %d %d %d %d %d %d\\n", SD_VP_MAX_SHARDS, SD_VP_MAX_BATCH, SD_VP_MAX_VOCAB_LOCAL, SD_VP_MAGIC,'
             ' SD_VP_STAT_OWNS, (int)SD_PATH_VERIFY_VP);\n  printf("abi %d\\n", SD_ABI_VERSION);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    for s in structs:
        assert int(got[f"{s}.size"]) == C.sizeof(getattr(_lib, s)), s
        for f, _ in getattr(_lib, s)._fields_:
            assert getattr(getattr(_lib, s), f).offset == int(got[f"{s}.{f}"]), (s, f)
    assert (C.sizeof(_lib.sd_vp_header), C.sizeof(_lib.sd_vp_stat), C.sizeof(_lib.sd_vp_cand)) == (32, 16, 32)
    assert got["limits"].split() == [str(v) for v in (_lib.SD_VP_MAX_SHARDS, _lib.SD_VP_MAX_BATCH,
                                                      _lib.SD_VP_MAX_VOCAB_LOCAL, _lib.SD_VP_MAGIC,
                                                      _lib.SD_VP_STAT_OWNS, _lib.SD_PATH_VERIFY_VP)]
    assert got["abi"] == "12" and _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12
    # additive: the existing structs keep the sizes they had before this entry point
    assert {s: int(got[f"{s}.size"]) for s in old} == {"sd_verify_args": 888, "sd_sample_args": 184,
                                                       "sd_ngram_args": 488, "sd_beam_args": 200,
                                                       "sd_multi_args": 816}
    for s in old:
        assert int(got[f"{s}.size"]) == C.sizeof(getattr(_lib, s)), s
    assert _lib.lib.sd_vp_stats_bytes(5, 4) == 32 + 5 * 9 * 16 and _lib.lib.sd_vp_cand_bytes(5) == 32 + 5 * 32
    assert _lib.lib.sd_vp_stats(None, None) == _lib.SD_ERR_INVALID


def test_vocab_shard_even_is_the_column_parallel_split():
    from specdec_amd.vocab_parallel import LocalShards, VocabShard
    for V, W in ((128256, 8), (50257, 3), (10, 4), (7, 7)):
        shards = [VocabShard.even(r, W, V) for r in range(W)]
        assert [s.vocab_local for s in shards] == vref.even_sizes(W, V)
        assert [s.vocab_offset for s in shards] == [o for o, _ in vref.bounds(vref.even_sizes(W, V))]
        LocalShards(shards)                                              # a partition, in order
    assert [s.vocab_local for s in VocabShard.split([2051, 2048, 1])] == [2051, 2048, 1]
    with pytest.raises(ValueError):
        VocabShard(0, 1, 0, 0, 8)
    with pytest.raises(ValueError):
        VocabShard(2, 2, 0, 4, 8)
    with pytest.raises(ValueError):
        LocalShards([VocabShard(0, 2, 0, 4, 8), VocabShard(1, 2, 5, 3, 8)])   # a gap


# ---------------------------------------------------------------- exactness by enumeration
SIZES7 = (1, 4, 2)


def _law_by_integration(w, sizes, greedy=False):
    """The law of pick()'s token over (u1, u2) ~ U[0, 1)^2, integrated exactly: pick() is piecewise
    constant, with breakpoints at the normalised prefix sums, so one evaluation per cell (at its
    midpoint) weighted by the cell's area."""
    w = np.asarray(w, dtype=np.float64)
    shard_iv, tok_iv = vref.intervals(w, sizes)
    M = shard_iv[-1, 1]
    cuts1 = np.unique(np.concatenate([[0.0, 1.0], shard_iv.reshape(-1) / M]))
    law = np.zeros(len(w))
    for a, b in zip(cuts1[:-1], cuts1[1:]):
        o = vref.pick(w, sizes, (a + b) / 2, 0.5, greedy).owner
        ms = shard_iv[o, 1] - shard_iv[o, 0]
        off, n = vref.bounds(sizes)[o]
        cuts2 = np.unique(np.concatenate([[0.0, 1.0], tok_iv[off:off + n].reshape(-1) / ms]))
        for c, d in zip(cuts2[:-1], cuts2[1:]):
            p = vref.pick(w, sizes, (a + b) / 2, (c + d) / 2, greedy)
            assert p.owner == o
            law[p.x] += (b - a) * (d - c)
    return law


def _rows7(seed):
    r = np.random.default_rng(seed)
    P = r.random((3, 7)) + 0.05
    Q = r.random((2, 7)) + 0.05
    P[:, 3] = 0.0                                        # a zero-weight token inside a slice
    return P / P.sum(-1, keepdims=True), Q / Q.sum(-1, keepdims=True)


def test_token_law_is_exact_at_a_residual_and_a_bonus_exit():
    """V = 7, S = 3 (slices 1/4/2): over every accept / reject branch (its probability from the accept
    uniforms) and the integral over (u1, u2), the emitted token at each exit follows w / Σw to 1e-12."""
    P, Q = _rows7(5)
    seen = set()
    ratio = np.where(P[:2] > 0, P[:2] / Q, np.inf)
    lo = [int(np.argmin(ratio[d])) for d in range(2)]         # p/q < 1: both branches have mass
    assert all(0 < ratio[d, lo[d]] < 1 for d in range(2))
    for tok in (lo, [lo[0], 3], [0, 6]):                      # token 3 has p = 0: always rejected
        for pr, o in mref.enumerate_outcomes(P[None], Q[None], np.array([tok])):
            law = _law_by_integration(o.weights, SIZES7)
            want = o.weights / o.weights.sum()
            assert abs(law.sum() - 1) < 1e-12
            assert np.abs(law - want).max() < 1e-12, (tok, o.status, np.abs(law - want).max())
            assert law[3] == 0 or o.weights[3] > 0
            seen.add(o.status)
    assert seen == {mref.RESIDUAL, mref.BONUS}
    # a slice without mass is never picked, wherever u1 falls
    w = np.array([0.0, 0.2, 0.0, 0.3, 0.1, 0.0, 0.0])
    law = _law_by_integration(w, SIZES7)
    assert np.abs(law - w / w.sum()).max() < 1e-12 and law[0] == 0 and law[5] == law[6] == 0
    for u1 in (0.0, 0.5, 1 - 2.0 ** -53):
        assert vref.pick(w, SIZES7, u1, 0.999).owner == 1


def test_greedy_is_the_global_argmax_lowest_index_first():
    w = np.array([0.1, 0.05, 0.3, 0.05, 0.3, 0.1, 0.1])       # the tie 2 / 4 sits inside slice 1
    assert vref.pick(w, SIZES7, 0.9, 0.9, greedy=True).x == 2
    w = np.array([0.05, 0.05, 0.1, 0.05, 0.3, 0.3, 0.15])     # the tie 4 / 5 straddles the slice boundary
    p = vref.pick(w, SIZES7, 0.9, 0.9, greedy=True)
    assert (p.x, p.owner) == (4, 1)
    w = np.array([0.3, 0.05, 0.1, 0.05, 0.1, 0.3, 0.1])       # the one-element slice ties with the last slice
    p = vref.pick(w, SIZES7, 0.1, 0.1, greedy=True)
    assert (p.x, p.owner) == (0, 0)
    for sizes in ((7,), (3, 4), (1, 1, 1, 1, 1, 1, 1)):
        assert vref.pick(w, sizes, 0.5, 0.5, greedy=True).x == 0


# ---------------------------------------------------------------- independence from the sharding
@pytest.mark.parametrize("case", [c for c in vc.grid() if c[2] == 4100 and c[1] in (0, 4)], ids=vc.case_id)
def test_decisions_do_not_depend_on_the_sharding(case):
    c = vc.case(*case)
    V = c.V
    base = vc.host_results(c, sizes=(V,))
    splits = [(V,), (V // 2, V - V // 2), (1, V - 1), tuple(vref.even_sizes(3, V)), (2051, 2048, 1),
              tuple(vref.even_sizes(8, V)), (1, 1, 1, 1, 1, 1, 1, V - 7)]
    for sizes in splits:
        for a, r in zip(base, vc.host_results(c, sizes=sizes)):
            assert (r.n, r.status, r.stop_index, r.prune_drafter, r.prune_target) == \
                (a.n, a.status, a.stop_index, a.prune_drafter, a.prune_target)
            assert r.resample_mass == a.resample_mass or (np.isnan(r.resample_mass) and np.isnan(a.resample_mass))
            assert r.close == a.close
            if r.status != mref.STOP:
                assert abs(r.M - a.M) <= 1e-12 * max(a.M, 1.0)


def test_gamma_zero_samples_the_one_target_row():
    P, _ = _rows7(9)
    r = vref.step(P[:1], np.zeros((0, 7)), [], 77, 3, 5, SIZES7)
    assert (r.n, r.status, r.prune_drafter, r.prune_target, r.stop_index) == (0, mref.BONUS, 0, 0, -1)
    assert np.isnan(r.resample_mass) and np.array_equal(r.weights, P[0])
    lo, hi = r.prefix
    assert lo <= r.u1 * r.M < hi
    lo, hi = r.inner
    assert lo <= r.u2 * r.masses[r.owner] < hi and P[0, r.x] > 0


# ---------------------------------------------------------------- coverage of the GPU cases
@pytest.fixture(scope="module")
def grid_coverage():
    tot = None
    per_case = []
    for case in vc.grid():
        c = vc.case(*case)
        cov = vc.coverage(c, vc.host_results(c))
        per_case.append((case, cov))
        if tot is None:
            tot = cov
        else:
            for k, v in vars(cov).items():
                setattr(tot, k, getattr(tot, k) + v)
    return tot, per_case


def test_gpu_grid_holds_the_issue_shapes():
    g = vc.grid()
    assert {(c[2], c[3]) for c in g} == set(vc.LAYOUTS) | {vc.BIG}
    for V, sizes in vc.LAYOUTS:
        mine = [c for c in g if c[2] == V]
        assert {c[1] for c in mine} == {0, 1, 4, 32}
        assert {c[4] for c in mine} == set(vc.DTYPES) and {c[5] for c in mine} == set(vc.PROCS)
    assert {c[0] for c in g} == {1, 5, 16}
    assert {c[4] for c in g if c[2] == 128256} == set(vc.DTYPES)
    assert any(c[6] for c in g) and any(c[7] for c in g)


def test_gpu_cases_reach_every_branch(grid_coverage):
    tot, per_case = grid_coverage
    print(vars(tot))
    assert tot.rej0 >= 1 and tot.rej_deep >= 1 and tot.bonus >= 1 and tot.stop >= 1
    assert tot.tok_first >= 1 and tot.tok_last >= 1 and tot.one_elem_owner >= 1
    assert tot.owner_first >= 1 and tot.owner_last >= 1 and tot.owner_mid >= 1
    assert tot.dead_slices >= 1


def test_no_gpu_case_has_more_than_one_close_row(grid_coverage):
    """The cap the GPU comparison relies on, proved on the host model alone."""
    for case, cov in grid_coverage[1]:
        assert cov.close <= 1, (vc.case_id(case), cov.close)


# ---------------------------------------------------------------- exchange plumbing (two gloo ranks)
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _blocks(n):
    return [(torch.arange(n, dtype=torch.int64) * (7 + 13 * r) % 251).to(torch.uint8) for r in range(2)]


def _exchange_worker(rank, port, n, out):
    import torch.distributed as dist
    from specdec_amd.vocab_parallel import GroupExchange
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        got = GroupExchange(dist.group.WORLD)(_blocks(n)[rank])
        out.put((rank, got.tolist()))
    finally:
        dist.destroy_process_group()


def test_group_exchange_returns_the_blocks_in_rank_order():
    import torch.multiprocessing as mp
    from specdec_amd.vocab_parallel import LocalShards
    n = 32 + 5 * 9 * 16
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, port, n, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    want = LocalShards.concat(_blocks(n))
    assert want.shape == (2, n) and want.dtype == torch.uint8
    assert got[0] == want.tolist() and got[1] == want.tolist()


def test_a_wrong_exchange_result_is_a_value_error_not_a_kernel_call():
    from specdec_amd.vocab_parallel import _check_gathered
    dev = torch.device("cpu")
    ok = torch.zeros(3, 64, dtype=torch.uint8)
    assert _check_gathered(ok, 3, 64, dev, "statistics") is ok
    for bad in (torch.zeros(2, 64, dtype=torch.uint8), torch.zeros(3, 63, dtype=torch.uint8),
                torch.zeros(3, 64, dtype=torch.int8), torch.zeros(3, 128, dtype=torch.uint8)[:, ::2], None, [ok]):
        with pytest.raises(ValueError):
            _check_gathered(bad, 3, 64, dev, "statistics")


def test_user_processors_and_keep_processors_are_refused():
    from specdec_amd.utils.logits_processor import MultinomialProcessor, NucleusProcessor, TopKProcessor
    from specdec_amd.vocab_parallel import _vp_spec

    class Own(MultinomialProcessor):
        def _process(self, logits):
            return logits

    for proc in (Own(1.0), TopKProcessor(1.0, 50), NucleusProcessor(1.0, 0.9)):
        with pytest.raises(TypeError):
            _vp_spec(proc)
    assert _vp_spec(MultinomialProcessor(0.7)).temperature == pytest.approx(0.7)
    # the loop names the limit before it touches a model
    from specdec_amd.sampling import vocab_parallel_speculative_generate
    for proc in (Own(1.0), TopKProcessor(1.0, 50)):
        with pytest.raises(TypeError, match="vocabulary-parallel"):
            vocab_parallel_speculative_generate([1, 2], None, None, None, None, logits_processor=proc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_vp_ops_fake_shapes(dtype):
    import specdec_amd  # noqa: F401  (registers the ops)
    from specdec_amd import _lib
    from specdec_amd.vocab_parallel import VP_FIELDS
    B, g, Vs, S = 3, 5, 16032, 8
    t = torch.empty(B, g + 1, Vs, device="meta", dtype=dtype)
    d = torch.empty(B, g, Vs, device="meta", dtype=dtype)
    tok = torch.empty(B, g, device="meta", dtype=torch.long)
    stops = torch.empty(2, device="meta", dtype=torch.long)
    op = torch.ops.specdec
    stats = op.vp_stats(t, d, tok, 3, S, 3 * Vs, 128256, 1, 0.7)
    assert (stats.shape, stats.dtype, stats.device.type) == ((_lib.lib.sd_vp_stats_bytes(B, g),), torch.uint8, "meta")
    cand = op.vp_decide(t, d, tok, stops, stats.new_empty(S, stats.shape[0]), 3, S, 3 * Vs, 128256, 1, 0.7, False, 7, 0, 0)
    assert (cand.shape, cand.dtype, cand.device.type) == ((_lib.lib.sd_vp_cand_bytes(B),), torch.uint8, "meta")
    out = op.vp_finish(cand.new_empty(S, cand.shape[0]), g, 3, S, 3 * Vs, Vs, 128256, 1, 7, 0, 0)
    assert len(out) == len(VP_FIELDS) == 8
    want = {"next_token": torch.long, "resample_mass": torch.float32}
    for f, o in zip(VP_FIELDS, out):
        assert (o.shape, o.dtype, o.device.type) == ((B,), want.get(f, torch.int32), "meta"), f
