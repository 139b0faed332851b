"""GPU tests of the dynamic draft trees' growth and rerank (sd_tree_grow, sd_tree_select;
csrc/tree_grow.hip) against the host model (tests/tree_dynamic_ref.py, fp64) on the cases of
tests/tree_dynamic_cases.py: tokens, parents, depths, pool indices and ancestor sets exactly, scores
within 1e-4.  The cases' input seeds are chosen on the host so that no frontier or final-N boundary is
within 1e-3 of a tie (tests/test_tree_dynamic_cpu.py checks that such seeds exist): exact equality is a
fair demand there.  Plus exact ties, -inf entries, c = V, a NaN row, poisoned buffers, graph capture
and the torch ops."""
import math
from types import SimpleNamespace

import pytest
import torch

import row_edges as rowe
import tree_dynamic_cases as yc
import tree_dynamic_ref as yref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 3                                   # sentinel columns behind every pool row
TOK_POISON, PAR_POISON = -99, -77


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.tree import DynamicTreeSpec
    return SimpleNamespace(lib=_lib, ops=ops, Spec=DynamicTreeSpec)


def poisoned_pool(B, P):
    """(pool over views [B, P], the three whole buffers [B, P + PAD])."""
    bufs = (torch.full((B, P + PAD), TOK_POISON, dtype=torch.long, device=DEV),
            torch.full((B, P + PAD), math.nan, dtype=torch.float32, device=DEV),
            torch.full((B, P + PAD), PAR_POISON, dtype=torch.int32, device=DEV))
    return SimpleNamespace(token=bufs[0][:, :P], score=bufs[1][:, :P], parent=bufs[2][:, :P]), bufs


def assert_poison(bufs, P):
    assert bool((bufs[0][:, P:] == TOK_POISON).all()) and bool(bufs[1][:, P:].isnan().all()) \
        and bool((bufs[2][:, P:] == PAR_POISON).all())


def grow_all(sd, rows, W, c, layout="packed", status_or=None):
    """Every level on the device: (pool, its buffers, the per-level outputs)."""
    B, L = rows[0].shape[0], len(rows)
    P = sd.Spec(L, W, c, 1).pool_size
    pool, bufs = poisoned_pool(B, P)
    outs, front = [], None
    for level, x in enumerate(rows, 1):
        x = rowe.place(x, layout, math.nan, DEV)
        front = sd.ops.tree_grow(x, level, W, c, pool, None if front is None else front.pool, status_or=status_or)
        outs.append(front)
    return pool, bufs, outs


def check_scores(got, want, what):
    got, want = got.double().cpu(), torch.tensor(want, dtype=torch.float64)
    inf = want == -math.inf
    assert torch.equal(got == -math.inf, inf), what
    dev = float((got[~inf] - want[~inf]).abs().max()) if bool((~inf).any()) else 0.0
    print(f"[tree-grow] {what}: max |score - fp64| = {dev:.3g} (bound {yref.SCORE_TOL})")
    assert dev <= yref.SCORE_TOL, (what, dev)


def check_sequence(sd, b, m, pool, outs, sel, what):
    L = sd.lib
    for lv, (got, want) in enumerate(zip(outs, m.grow.frontiers), 1):
        assert got.token[b].tolist() == want.token, (what, b, lv)
        assert got.pool[b].tolist() == want.pool, (what, b, lv)
        assert got.parent_rank[b].tolist() == want.parent_rank, (what, b, lv)
        assert int(got.row_status[b]) == L.SD_ROW_DONE, (what, b, lv)
    assert pool.token[b].tolist() == m.grow.pool.token, (what, b)
    assert pool.parent[b].tolist() == m.grow.pool.parent, (what, b)
    check_scores(pool.score[b], m.grow.pool.score, f"{what} b={b}")
    if sel is not None:
        assert sel.tokens[b].tolist() == m.sel.tokens, (what, b)
        assert sel.parent[b].tolist() == m.sel.parent, (what, b)
        assert sel.depth[b].tolist() == m.sel.depth, (what, b)
        assert sel.pool_index[b].tolist() == m.sel.pool_index, (what, b)
        assert [a & ((1 << 64) - 1) for a in sel.anc[b].tolist()] == m.sel.anc, (what, b)
        assert int(sel.row_status[b]) == L.SD_ROW_DONE, (what, b)


def run_case(sd, c, layout):
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pool, bufs, outs = grow_all(sd, c.rows, c.W, c.c, layout, err)
    P = pool.token.shape[1]
    sel = sd.ops.tree_select(pool, c.N, status_or=err)
    what = f"V{c.V}-B{c.B}-W{c.W}c{c.c}-L{c.L}-N{c.N}-{rowe.dt_name(c.dtype)}-{layout}-seed{c.seed}"
    for b, m in enumerate(c.models):
        check_sequence(sd, b, m, pool, outs, sel, what)
    assert_poison(bufs, P)
    assert int(err[0]) == 0
    return pool, sel


def _id(g):
    V, B, W, c, L, N, dt, layout = g
    return f"V{V}-B{B}-W{W}c{c}-L{L}-N{N}-{rowe.dt_name(dt)}-{layout}"


@pytest.mark.parametrize("g", yc.grid(), ids=_id)
def test_grow_and_select_equal_the_host_model(sd, g):
    run_case(sd, yc.case(*g[:7]), g[7])


@pytest.mark.parametrize("g", [(2049, 3, 8, 8, 2, 64, torch.bfloat16), (4097, 1, 2, 3, 5, 7, torch.float32)], ids=["bf16", "f32"])
def test_rows_with_minus_infinity_entries(sd, g):
    """Half of every row at -inf: such tokens are ordinary candidates that sort last (c = 8 of a 5-token
    finite set would reach them; here they stay out of every top-c) and -inf never becomes NaN."""
    c = yc.case(*g, mask=True)
    pool, _ = run_case(sd, c, "shifted")
    assert bool(torch.isfinite(pool.score).all())


def test_minus_infinity_candidates_are_pool_entries_that_sort_last(sd):
    """V = 8 with only 3 finite logits and c = 5: two children of every row have score -inf.  They enter
    the pool, lose every comparison, and tie among themselves by pool index."""
    V, W, c = 8, 4, 5
    g = torch.Generator().manual_seed(3)
    rows = []
    for F in (1, 4):
        x = torch.full((2, F, V), -math.inf)
        x[:, :, [1, 4, 6]] = torch.randn(2, F, 3, generator=g) * 3
        rows.append(x)
    models = yc.host(rows, W, c, 12)
    assert not any(m.close for m in models)
    assert all(sum(s == -math.inf for s in m.grow.pool.score) == 2 + 3 * 2 + 5 for m in models)   # and the five under a -inf parent
    pool, bufs, outs = grow_all(sd, rows, W, c)
    sel = sd.ops.tree_select(pool, 12)
    for b, m in enumerate(models):
        check_sequence(sd, b, m, pool, outs, sel, "minus-inf")
    # N reaches into the -inf entries: 3 + 9 finite candidates, then -inf ones by pool index
    sel = sd.ops.tree_select(pool, 17)
    for b in range(2):
        m = yref.select(models[b].grow.pool, 17)
        assert sel.pool_index[b].tolist() == m.pool_index and sel.parent[b].tolist() == m.parent and m.closed


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_ties_resolve_by_pool_index(sd, dtype):
    """Two equal maxima in the root's row (equal parent scores), then two IDENTICAL frontier rows: the
    candidates tie pairwise exactly, on the device as on the host, and the lower pool index wins."""
    W, c = 2, 2
    r0 = torch.tensor([[[1.0, 5.0, 0.0, 5.0, -1.0, 0.0, 0.0, 0.0]]]).to(dtype)
    r1 = torch.tensor([[[0.0, 2.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0]] * 2]).to(dtype)
    m = yref.model([r0[0], r1[0]], W, c, 4)
    assert m.grow.frontiers[1].pool == [2, 4] and m.sel.pool_index == [0, 1, 2, 4] and not m.close
    pool, bufs, outs = grow_all(sd, [r0, r1], W, c)
    sel = sd.ops.tree_select(pool, 4)
    check_sequence(sd, 0, m, pool, outs, sel, "ties")
    s = pool.score[0].tolist()
    assert s[0] == s[1] and s[2] == s[4] and s[3] == s[5]
    sel3 = sd.ops.tree_select(pool, 3)                       # the boundary falls inside the tie of 2 and 4
    assert sel3.pool_index[0].tolist() == [0, 1, 2] and sel3.parent[0].tolist() == [-1, -1, 0]
    # whole rows of one value: top-c is the lowest indices, across the chunk edge too
    x = torch.zeros(1, 1, 4097, dtype=dtype)
    pool, _, outs = grow_all(sd, [x], 8, 8)
    assert outs[0].token[0].tolist() == list(range(8)) and outs[0].pool[0].tolist() == list(range(8))
    x[0, 0, [2047, 2048, 4096]] = 1.0
    pool, _, outs = grow_all(sd, [x], 8, 8)
    assert outs[0].token[0].tolist() == [2047, 2048, 4096, 0, 1, 2, 3, 4]


def test_branch_equal_to_the_vocabulary(sd):
    V = 8
    g = torch.Generator().manual_seed(5)
    for seed in range(16):
        g.manual_seed(seed)
        rows = [torch.randn(3, 1, V, generator=g) * 3, torch.randn(3, 8, V, generator=g) * 3]
        models = yc.host(rows, 8, 8, 64)
        if not any(m.close for m in models):
            break
    pool, bufs, outs = grow_all(sd, rows, 8, 8)
    sel = sd.ops.tree_select(pool, 64)
    for b, m in enumerate(models):
        check_sequence(sd, b, m, pool, outs, sel, "c=V")
        assert sorted(pool.token[b, :8].tolist()) == list(range(V))
    assert_poison(bufs, 72)


def test_a_nan_row_flags_its_sequence_only(sd):
    L = sd.lib
    c = yc.case(2049, 3, 8, 8, 2, 64, torch.bfloat16)
    rows = [r.clone() for r in c.rows]
    rows[1][1, 5, 2048] = math.nan                          # sequence 1, level 2, frontier row 5, the short last chunk
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pool, bufs, outs = grow_all(sd, rows, c.W, c.c, "padded", err)
    sel = sd.ops.tree_select(pool, c.N, status_or=err)
    assert int(outs[0].row_status[1]) == L.SD_ROW_DONE
    assert int(outs[1].row_status[1]) & L.SD_ROW_INVALID_DIST and int(err[0]) & L.SD_ROW_INVALID_DIST
    assert int(sel.row_status[1]) & L.SD_ROW_INVALID_DIST   # NaN scores reached the pool
    for b in (0, 2):
        check_sequence(sd, b, c.models[b], pool, outs, sel, "nan-others")
    # the flagged sequence's outputs stay inside their buffers and in range
    assert_poison(bufs, pool.token.shape[1])
    assert bool(((sel.pool_index[1] >= 0) & (sel.pool_index[1] < 72)).all())
    assert bool(((outs[1].pool[1] >= 8) & (outs[1].pool[1] < 72)).all())
    assert bool(((pool.token[1] >= 0) & (pool.token[1] < c.V)).all())
    # an all -inf row and a +inf are flagged too
    for bad in (-math.inf, math.inf):
        x = torch.randn(2, 1, 300)
        x[1, 0] = bad if bad < 0 else x[1, 0]
        x[1, 0, 7] = bad
        p2, _ = poisoned_pool(2, 4)
        out = sd.ops.tree_grow(x.to(DEV), 1, 2, 4, p2)
        assert int(out.row_status[0]) == L.SD_ROW_DONE and int(out.row_status[1]) & L.SD_ROW_INVALID_DIST


def test_a_level_captured_in_a_graph_equals_eager(sd):
    c = yc.case(4097, 3, 8, 8, 2, 64, torch.float32)
    other = yc.rows_of(c.seed + 100, c.B, c.V, c.W, c.c, c.L, c.dtype)
    x0, x1 = c.rows[0].to(DEV), c.rows[1].to(DEV)
    pool, _ = poisoned_pool(c.B, 72)
    f1 = sd.ops.tree_grow(x0, 1, 8, 8, pool)
    fin = f1.pool.clone()
    eager = sd.ops.tree_grow(x1, 2, 8, 8, pool, fin)          # sizes the workspace
    want = [t.clone() for t in (eager.token, eager.pool, eager.parent_rank, pool.token, pool.score, pool.parent)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sd.ops.tree_grow(x1, 2, 8, 8, pool, fin)
    # replay on other rows, then on the case's again
    x1.copy_(other[1].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out.token, want[0])
    x1.copy_(c.rows[1].to(DEV))
    pool.token[:, 8:].fill_(TOK_POISON)
    graph.replay()
    torch.cuda.synchronize()
    got = (out.token, out.pool, out.parent_rank, pool.token, pool.score, pool.parent)
    for g_, w in zip(got, want):
        assert torch.equal(g_, w)


def test_torch_ops_equal_the_python_api(sd):
    c = yc.case(2049, 3, 8, 8, 2, 64, torch.bfloat16)
    pool, _, outs = grow_all(sd, c.rows, c.W, c.c)
    sel = sd.ops.tree_select(pool, c.N)
    p2, _ = poisoned_pool(c.B, 72)
    a = torch.ops.specdec.tree_grow(c.rows[0].to(DEV), 1, 8, 8, p2.token, p2.score, p2.parent, None)
    b = torch.ops.specdec.tree_grow(c.rows[1].to(DEV), 2, 8, 8, p2.token, p2.score, p2.parent, a[1])
    for got, want in zip(b, (outs[1].token, outs[1].pool, outs[1].parent_rank, outs[1].row_status)):
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(p2.token, pool.token) and torch.equal(p2.score, pool.score) and torch.equal(p2.parent, pool.parent)
    s = torch.ops.specdec.tree_select(p2.token, p2.score, p2.parent, c.N, 72)
    for got, f in zip(s, ("tokens", "parent", "depth", "pool_index", "anc", "row_status")):
        assert torch.equal(got, getattr(sel, f)), f


def test_select_over_the_largest_pool(sd):
    """A full pool of 2048 entries (more than one entry per thread), random scores with a parent-closed
    structure: a chain of pool entries i -> i - 1 with decreasing scores, so the best N are the first N."""
    B, P, N = 2, 2048, 64
    g = torch.Generator().manual_seed(9)
    score = -torch.rand(B, P, generator=g).cumsum(1)
    parent = (torch.arange(P) - 1).expand(B, P).contiguous().int()
    tok = torch.randint(0, 1000, (B, P), generator=g)
    pool = SimpleNamespace(token=tok.to(DEV), score=score.to(DEV), parent=parent.to(DEV))
    sel = sd.ops.tree_select(pool, N)
    assert sel.pool_index.tolist() == [list(range(N))] * B and sel.parent.tolist() == [list(range(-1, N - 1))] * B
    assert sel.depth.tolist() == [list(range(1, N + 1))] * B and torch.equal(sel.tokens.cpu(), tok[:, :N])
    assert [a & ((1 << 64) - 1) for a in sel.anc[0].tolist()] == [(1 << (i + 1)) - 1 for i in range(N)]
    # a star: every entry a child of the root, random scores: the N best by (score, index) in index order
    parent = torch.full((B, P), -1, dtype=torch.int32)
    score = -torch.rand(B, P, generator=g)
    score[:, 2047] = 0.0                                     # the last entry of the last thread's slice is the best
    pool = SimpleNamespace(token=tok.to(DEV), score=score.to(DEV), parent=parent.to(DEV))
    sel = sd.ops.tree_select(pool, N)
    for b in range(B):
        want, _ = yref.best_of(score[b].double().tolist(), N)
        assert sel.pool_index[b].tolist() == want and want[-1] == 2047
    assert bool((sel.depth == 1).all()) and bool((sel.parent == -1).all())
