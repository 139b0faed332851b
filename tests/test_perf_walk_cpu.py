"""The reference side of tests/test_gpu_gamma_edges.py, alone and without a GPU: the conditions that
keep those GPU tests from passing vacuously are proven here for exactly the cases, rules, seeds and
offsets that file runs (its case lists are imported, so the two cannot drift), and the host model
itself (tests/perf_walk.py, tests/philox_ref.py) is guarded against the bugs it is meant to catch.
"""
import numpy as np
import pytest
import torch

import perf_walk as pw
import philox_ref as ph
import test_gpu_gamma_edges as ge


def case_problems(c, n_ends=0):
    """What is wrong with walk case c as a test input (empty: nothing)."""
    case, ends, late, rows = ge.host_side(c, n_ends)
    cov = pw.coverage(case, rows)
    g, bad = c.gamma, []
    if cov.close:
        bad.append(f"{cov.close} close rows")
    if cov.widened > 1:
        bad.append(f"{cov.widened} rows with a widened chunk bracket")
    if c.kind == "long":
        if cov.mid4 < 8:
            bad.append(f"only {cov.mid4} comparisons at index >= 4 with ratio in [0.1, 0.9]")
        if cov.full < 1:
            bad.append("no full accept")
        if cov.early_rej < 1:
            bad.append("no reject before index 4")
    else:
        for k in pw.pivots(g):
            if cov.pivot_mid.get(k, 0) < 2:
                bad.append(f"pivot {k} reached by {cov.pivot_mid.get(k, 0)} rows with ratio in [0.1, 0.9]")
        if g >= 5 and not (cov.acc4 and cov.rej4):
            bad.append(f"index >= 4: {cov.acc4} accepts, {cov.rej4} rejects")
        if g >= 9 and not (cov.acc8 and cov.rej8):
            bad.append(f"index >= 8: {cov.acc8} accepts, {cov.rej8} rejects")
    if c.rule == "engine" and g >= 5:
        if late is None:
            bad.append("no accepted draft at index >= 4 to end a row with")
        elif not (rows[late[0]].finished and rows[late[0]].want == late[1] + 1):
            bad.append("the late end token does not finish its row there")
    return bad


ALL_WALKS = [(c, 0) for c in ge.WALK_CASES] + [(c, n) for c in ge.END_CASES for n in (65, 300)]


@pytest.mark.parametrize("c,n_ends", ALL_WALKS, ids=[f"{c.id}-ends{n}" if n else c.id for c, n in ALL_WALKS])
def test_gpu_walk_cases_cover_what_they_claim(c, n_ends):
    assert case_problems(c, n_ends) == []


def test_gpu_walk_cases_expect_the_selected_kernel():
    """The dispatch model the GPU file asserts paths with: a selection names the kernel it gets wherever
    that kernel takes the shape, and γ = 9 at B = 8 is the first shape past the lean kernel."""
    from types import SimpleNamespace
    lib = SimpleNamespace(SD_PATH_VERIFY_LEAN=1, SD_PATH_VERIFY_FUSED=2, SD_PATH_VERIFY_TWO_LAUNCH=3,
                          SD_PATH_VERIFY_FUSED_TICKET=5)
    seen = set()
    for c in ge.WALK_CASES:
        n_t = c.gamma + (c.rule == "spec")
        for B in ((c.B // 2,) if c.shards else (c.B,)):
            p = ge.expected_path(lib, c, B)
            seen.add((c.sel, p))
            if c.sel == "lean":
                assert p == lib.SD_PATH_VERIFY_LEAN
            elif c.sel == "two-launch":
                assert p == lib.SD_PATH_VERIFY_TWO_LAUNCH
            elif c.sel == "default":
                assert p == lib.SD_PATH_VERIFY_FUSED_TICKET
            else:
                fused = lib.SD_PATH_VERIFY_FUSED_TICKET if c.sel == "ticket" else lib.SD_PATH_VERIFY_FUSED
                assert p == (fused if n_t <= ge.FUSED_MAX_TSLOTS else lib.SD_PATH_VERIFY_TWO_LAUNCH)
    edge = [c for c in ge.WALK_CASES if c.B == 8 and c.gamma == 9 and c.sel == "fused"]
    assert edge and all(ge.expected_path(lib, c, 8) == lib.SD_PATH_VERIFY_FUSED for c in edge)
    assert {c.gamma for c in ge.WALK_CASES if c.kind == "edge" and not c.shards and not c.row_base
            and c.sel in ("fused", "ticket", "two-launch") and c.B == 16 and c.V == 4096} == set(ge.GAMMAS)


def test_edge_walk_case_is_what_it_says():
    B, g, V = 8, 9, 2048
    tl, dl, ids, k = pw.edge_walk_case(B, g, V, torch.bfloat16, 3)
    case = pw.walk_case("edge", B, g, V, torch.bfloat16, 3)
    assert k == [pw.pivots(g)[b % 5] for b in range(B)] and pw.pivots(g) == [0, 3, 4, 7, 8]
    for b in range(B):
        assert torch.equal(dl[b, :k[b]], tl[b, :k[b]])                     # bit for bit
        assert not torch.equal(dl[b, k[b]], tl[b, k[b]])
        for i in range(g):
            p, q = float(case.P[b, i, ids[b, i]]), float(case.Q[b, i, ids[b, i]])
            if i < k[b]:
                assert p == q and int(ids[b, i]) == int(tl[b, i].float().argmax())
            else:
                assert q >= 1e-4 and 0.4 <= p / q <= 0.6
    # ratio exactly 1: SPEC never rejects, ENGINE always accepts, whatever the uniform
    for b in range(B):
        rows_s = pw.host_rows(case, "spec", 1, 2)[b]
        rows_e = pw.host_rows(case, "engine", 1, 2)[b]
        assert rows_s.want >= k[b] and rows_e.want >= k[b]


@pytest.mark.parametrize("seed,off,row", [(0x1234_5678_9ABC, 5, 0), (99, 1 << 33, 7), (99, 1 << 33, 1015)])
def test_accept_uniform_reads_block_i_over_4(seed, off, row):
    """Draft i's uniform is word i & 3 of block i >> 2 — and not block 0's word at i & 3, which a model
    (or a kernel) that ignores the block index would use."""
    for i in range(4, 32):
        blk = ph.block(seed, off, row, ph.SITE_ACCEPT, i >> 2)
        w = int(blk[i & 3])
        assert ph.accept_uniform(seed, off, row, i) == np.float32((w & 0xFFFFFF) * 2.0 ** -24)
        w0 = int(ph.block(seed, off, row, ph.SITE_ACCEPT, 0)[i & 3])
        assert w != w0 and ph.accept_uniform(seed, off, row, i) != ph.accept_uniform(seed, off, row, i & 3)


def direct_pick(weights, t, width):
    """numpy reference of the chunk pick at threshold t: searchsorted over the fp64 cumulative masses of
    the chunks that have any."""
    V = len(weights)
    mass = np.add.reduceat(weights, np.arange(0, V, width))
    pos = np.nonzero(mass > 0)[0]
    j = np.searchsorted(np.cumsum(mass[pos]), t, side="right")
    return int(pos[min(j, len(pos) - 1)])


@pytest.mark.parametrize("V", [2048, 4096, 6149, 50257])
@pytest.mark.parametrize("holes", [False, True], ids=["dense", "empty-edge-chunks"])
def test_chunk_bracket_against_searchsorted(V, holes):
    rng = np.random.default_rng(V + holes)
    width, tol = pw.CHUNK_WIDTH, pw.MASS_TOL
    w = rng.random(V) ** 4
    n_chunks = -(-V // width)
    if holes and n_chunks >= 3:          # leading and trailing chunks without mass, and one inside
        w[:width] = 0
        w[(n_chunks - 1) * width:] = 0
        if n_chunks > 4:
            w[2 * width:3 * width] = 0
    elif holes:
        w[: V // 2] = 0
    total = np.add.reduceat(w, np.arange(0, V, width)).sum()
    us = np.concatenate([[0.0, 1.0 - 2.0 ** -53], rng.random(10_000)])
    widened = 0
    for u in us:
        lo, hi = pw.chunk_bracket(w, u)
        want = direct_pick(w, u * total, width)
        assert lo <= want <= hi and w[want * width:(want + 1) * width].sum() > 0
        assert (lo, hi) == (direct_pick(w, (u - tol) * total, width), direct_pick(w, (u + tol) * total, width))
        widened += lo != hi
    assert widened < 0.01 * len(us)
    lo, hi = pw.chunk_bracket(w, 0.0)
    assert lo == hi == direct_pick(w, 0.0, width)
    assert pw.chunk_bracket(w, 1.0 - 2.0 ** -53)[1] == int(np.nonzero(np.add.reduceat(w, np.arange(0, V, width)) > 0)[0][-1])


def test_chunk_bracket_widens_only_at_a_boundary():
    w = np.ones(4 * 2048)
    assert pw.chunk_bracket(w, 0.25 + 2e-5) == (1, 1)
    assert pw.chunk_bracket(w, 0.25 - 2e-5) == (0, 0)
    assert pw.chunk_bracket(w, 0.25 + 5e-6) == (0, 1)
    assert pw.chunk_bracket(w, 0.25 - 5e-6) == (0, 1)
    assert pw.chunk_bracket(w[:100], 0.7) == (0, 0)
