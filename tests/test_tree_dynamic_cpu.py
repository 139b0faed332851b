"""CPU checks of the dynamic draft trees (sd_tree_grow, sd_tree_select, sd_verify_tree_dynamic; DESIGN.md
§4g): the ctypes mirrors against the header, the host model (tests/tree_dynamic_ref.py) against an
independent brute-force enumeration of the EAGLE-2 pool, the invariants the verify's ABI asks of a
selected tree, losslessness of the rule on trees grown per context by exact enumeration, the Python
shape helpers, the ops' fake implementations and the status of refused calls (no launch: every call
here is refused before one)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import tree_distinct_ref as dref
import tree_dynamic_ref as yref
from tree_ref import children_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sd_tree_grow_args", "sd_tree_select_args", "sd_tree_dynamic_args")


# ---------------------------------------------------------------- struct layout, constants, exports
def test_new_structs_ctypes_layout_matches_the_header():
    from specdec_amd import _lib
    old = ["sd_verify_args", "sd_sample_args", "sd_ngram_args", "sd_beam_args", "sd_multi_args", "sd_vp_args", "sd_tree_args",
           "sd_tree_distinct_args", "sd_kv_compact_args"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
    for s in NEW:
        prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
        for f, _ in getattr(_lib, s)._fields_:
            prog += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    for o in old:
        prog += f'  printf("{o}.size %zu\\n", sizeof({o}));\n'
    prog += ('  printf("path %d\\n", (int)SD_PATH_VERIFY_TREE_DYNAMIC);\n  printf("pool %d\\n", SD_TREE_POOL_MAX);\n'
             '  printf("width %d\\n", SD_TREE_GROW_MAX_WIDTH);\n  printf("vocab %d\\n", SD_TREE_GROW_MAX_VOCAB);\n'
             '  printf("abi %d\\n", SD_ABI_VERSION);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    for s in NEW:
        assert int(got[f"{s}.size"]) == C.sizeof(getattr(_lib, s)), s
        for f, _ in getattr(_lib, s)._fields_:
            assert getattr(getattr(_lib, s), f).offset == int(got[f"{s}.{f}"]), (s, f)
    # sd_tree_distinct_args with the host parent[] replaced by the device parents, their stride and max_depth
    same = lambda fs: [f for f in fs if f not in ("parent", "parent_dev", "parent_stride_b", "max_depth")]  # noqa: E731
    assert same([f for f, _ in _lib.sd_tree_dynamic_args._fields_]) == same([f for f, _ in _lib.sd_tree_distinct_args._fields_])
    assert got["path"] == "10" and _lib.SD_PATH_VERIFY_TREE_DYNAMIC == 10
    assert got["pool"] == "2048" and _lib.SD_TREE_POOL_MAX == 2048
    assert int(got["width"]) == _lib.SD_TREE_GROW_MAX_WIDTH == 8 and int(got["vocab"]) == _lib.SD_TREE_GROW_MAX_VOCAB
    assert got["abi"] == "12" and _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12
    for o in old:                                        # additive: the existing structs keep their sizes
        assert int(got[f"{o}.size"]) == C.sizeof(getattr(_lib, o)), o
    for name in ("sd_tree_grow", "sd_tree_grow_workspace_size", "sd_tree_select", "sd_tree_select_workspace_size",
                 "sd_verify_tree_dynamic", "sd_verify_tree_dynamic_workspace_size"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.SD_PATH_VERIFY_TREE_DYNAMIC in _lib.PATH_NAMES


def test_workspace_sizes_and_refused_calls():
    from specdec_amd import _lib
    L, lib = _lib, _lib.lib
    cnt = 8 << 20                                        # the common counter block comes first
    assert lib.sd_tree_grow_workspace_size(1, 128256, 3, 8, 8) >= cnt + 8 * 18 * 63 * 4
    assert lib.sd_tree_select_workspace_size(3, 264, 64) >= cnt
    assert lib.sd_verify_tree_dynamic_workspace_size(2, 28, 4096) == lib.sd_verify_tree_distinct_workspace_size(
        2, 28, (C.c_int32 * 64)(*range(-1, 27)), 4096)      # the size depends on N alone
    for bad in ((0, 64, 1, 1, 1), (1, 0, 1, 1, 1), (1, 64, 0, 1, 1), (1, 64, 33, 1, 1), (1, 64, 1, 0, 1), (1, 64, 1, 9, 1),
                (1, 64, 1, 1, 0), (1, 64, 1, 1, 9), (1, 4, 1, 1, 5), (1, (1 << 19) + 1, 1, 1, 1)):
        assert lib.sd_tree_grow_workspace_size(*bad) == 0, bad
    assert lib.sd_tree_grow_workspace_size(1, 64, 32, 8, 8) > 0           # the largest pool, 8 + 31 * 64 = 1992, fits
    for bad in ((0, 8, 1), (1, 0, 1), (1, 8, 0), (1, 2049, 1), (1, 8, 9), (1, 100, 65)):
        assert lib.sd_tree_select_workspace_size(*bad) == 0, bad
    for bad in ((0, 1, 64), (1, 0, 64), (1, 65, 64), (1, 1, 0), (16385, 1, 64)):
        assert lib.sd_verify_tree_dynamic_workspace_size(*bad) == 0, bad
    g = L.sd_tree_grow_args()
    assert lib.sd_tree_grow(C.byref(g), None) == L.SD_ERR_INVALID
    g.batch, g.vocab, g.level, g.width, g.branch = 1, 64, 1, 9, 2
    assert lib.sd_tree_grow(C.byref(g), None) == L.SD_ERR_UNSUPPORTED
    g.width, g.branch = 2, 65
    assert lib.sd_tree_grow(C.byref(g), None) == L.SD_ERR_UNSUPPORTED
    g.branch, g.vocab = 8, 4
    assert lib.sd_tree_grow(C.byref(g), None) == L.SD_ERR_INVALID         # c > V
    s = L.sd_tree_select_args()
    s.batch, s.pool_size, s.num_nodes = 1, 2049, 4
    assert lib.sd_tree_select(C.byref(s), None) == L.SD_ERR_UNSUPPORTED
    s.pool_size, s.num_nodes = 8, 9
    assert lib.sd_tree_select(C.byref(s), None) == L.SD_ERR_INVALID       # N > pool
    d = L.sd_tree_dynamic_args()
    d.batch, d.num_nodes, d.vocab, d.max_depth = 1, 4, 64, 0
    assert lib.sd_verify_tree_dynamic(C.byref(d), None) == L.SD_ERR_INVALID
    d.max_depth = 33
    d.dtype, d.proc.kind, d.proc.temperature, d.proc.top_p = L.SD_BF16, L.SD_PROC_MULTINOMIAL, 1.0, 1.0
    for f in ("parent_dev", "draft_tokens", "n_accepted", "last_node", "next_token", "row_status", "path"):
        setattr(d, f, 0x1000)
    d.noise.mode = L.SD_NOISE_PHILOX
    assert lib.sd_verify_tree_dynamic(C.byref(d), None) == L.SD_ERR_UNSUPPORTED


# ---------------------------------------------------------------- the host model against brute force
def _ctx_logits(seed, V):
    cache = {}

    def rows(ctx):
        if ctx not in cache:
            rng = np.random.default_rng([seed, len(ctx)] + [int(t) + 2 for t in ctx])
            cache[ctx] = rng.normal(size=V) * 2.0
        return cache[ctx]
    return rows


@pytest.mark.parametrize("V,L,W,c,N", [(4, 2, 2, 2, 3), (5, 3, 2, 3, 7), (16, 2, 8, 8, 64), (7, 3, 3, 2, 6), (3, 3, 1, 1, 3),
                                       (6, 1, 4, 6, 4), (16, 3, 4, 3, 20)])
def test_host_model_equals_a_brute_force_enumeration(V, L, W, c, N):
    for seed in range(8):
        rows = _ctx_logits(seed, V)
        g = yref.grow(lambda level, fr: torch.tensor(np.stack([rows(f.path) for f in fr])), L, W, c)
        N_ = min(N, len(g.pool.token))
        s = yref.select(g.pool, N_)
        chosen, fronts, cands = yref.brute_force(rows, V, L, W, c, N_)
        F, base = yref.shape(L, W, c)
        assert len(g.pool.token) == base[-1] == len(cands)
        assert {p: None for p in g.pool.path}.keys() == cands.keys()
        for p, sc in zip(g.pool.path, g.pool.score):
            assert abs(sc - cands[p]) < 1e-12
        for lv, want in zip(g.frontiers, fronts):
            assert {g.pool.path[i] for i in lv.pool} == want and lv.pool == sorted(lv.pool)
        assert set(s.path) == chosen and s.pool_index == sorted(s.pool_index)
        # the final parents reproduce the paths
        for i, p in enumerate(s.parent):
            assert s.path[i][:-1] == (s.path[p] if p >= 0 else ()) and s.tokens[i] == s.path[i][-1]


# ---------------------------------------------------------------- invariants of the selected tree
def _random_case(seed, V, L, W, c, ties, neg_inf):
    g = torch.Generator().manual_seed(seed)
    F, _ = yref.shape(L, W, c)
    rows = [torch.randn(F[l], V, generator=g) * 3 for l in range(L)]
    if ties:                                             # few distinct values: exact score ties everywhere
        rows = [torch.round(r) for r in rows]
        if L > 1 and F[1] > 1:
            rows[1][1] = rows[1][0]
    if neg_inf:
        for r in rows:
            r[:, torch.randperm(V, generator=g)[:max(1, V - c + 1 if seed % 2 else V // 2)]] = -math.inf
            r[:, 0] = 0.5                                # never a row without a finite element
    return rows


@pytest.mark.parametrize("ties,neg_inf", [(False, False), (True, False), (False, True), (True, True)])
def test_selected_trees_keep_the_verifys_invariants(ties, neg_inf):
    n = 0
    for seed in range(40):
        V, L, W, c = [(5, 2, 2, 3), (12, 5, 8, 8), (9, 3, 3, 2), (16, 4, 1, 1), (8, 2, 8, 8)][seed % 5]
        rows = _random_case(seed, V, L, W, c, ties, neg_inf)
        F, base = yref.shape(L, W, c)
        for N in {1, min(7, base[-1]), min(64, base[-1])}:
            m = yref.model(rows, W, c, N)
            s = m.sel
            assert s.closed, (seed, N)                   # parent-closed, also under ties and -inf scores
            assert all(-1 <= p < i for i, p in enumerate(s.parent))
            assert max(len(k) for k in children_of(s.parent)) <= c
            assert max(s.depth) <= L and min(s.depth) >= 1
            assert s.anc == yref.transitive_closure(s.parent)
            assert all(sc <= 0 or sc != sc for sc in m.grow.pool.score)
            # a child never scores above its parent, and lies above it in the pool
            for i, p in enumerate(m.grow.pool.parent):
                assert p < i and (p < 0 or m.grow.pool.score[i] <= m.grow.pool.score[p])
            n += 1
    assert n >= 80


def test_exact_ties_resolve_by_pool_index():
    V, W, c = 8, 2, 2
    r0 = torch.tensor([[1.0, 5.0, 0.0, 5.0, -1.0, 0.0, 0.0, 0.0]])         # tokens 1 and 3 tie: equal parent scores
    r1 = torch.tensor([[0.0, 2.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0]] * 2)       # two identical frontier rows
    m = yref.model([r0, r1], W, c, 4)
    assert m.grow.frontiers[0].token == [1, 3] and m.grow.pool.score[0] == m.grow.pool.score[1]
    assert m.grow.pool.score[2] == m.grow.pool.score[4] and m.grow.pool.score[3] == m.grow.pool.score[5]
    assert m.grow.frontiers[1].pool == [2, 4]            # the two 4s (score tie): lowest pool index first
    assert m.sel.pool_index == [0, 1, 2, 4] and m.sel.parent == [-1, -1, 0, 1]
    assert not m.close                                   # exact ties are not "close": both sides compute them equal


# ---------------------------------------------------------------- losslessness on trees grown per context
def _ctx_rows(seed, V=4):
    cache = {}

    def rows(ctx):
        if ctx not in cache:
            rng = np.random.default_rng([seed, len(ctx)] + [int(t) + 2 for t in ctx])
            y = rng.normal(size=V) * 1.5
            cache[ctx] = (np.exp(y) * rng.uniform(0.9, 1.1), rng.normal(size=V) * 1.5)     # p unnormalised, drafter logits
        return cache[ctx]
    return rows


def test_first_two_tokens_keep_the_target_joint_on_grown_trees():
    """V = 4, context-dependent p and q, the tree GROWN per context (W = 2, c = 2, L = 2, N = 3): which nodes
    exist depends on the drafter's scores, yet every branch of the walk summed with its exact probability
    gives the target's joint of the first two emitted tokens, to 1e-12."""
    V, shapes = 4, set()
    for seed in range(12):
        rows = _ctx_rows(seed)
        g = yref.grow(lambda level, fr: torch.tensor(np.stack([rows(f.path)[1] for f in fr])), 2, 2, 2)
        s = yref.select(g.pool, 3)
        shapes.add(tuple(s.parent))
        ctx = [()] + list(s.path)
        P = np.stack([rows(c)[0] for c in ctx])
        tok = np.array(s.tokens)
        norm = lambda c: rows(c)[0] / rows(c)[0].sum()  # noqa: E731
        want = np.array([[norm(())[a] * norm((a,))[b] for b in range(V)] for a in range(V)])
        got, total = np.zeros((V, V)), 0.0
        for pr, o in dref.enumerate_outcomes(P, tok, s.parent):
            total += pr
            acc = [int(tok[k]) for k in o.path]
            last = o.weights / o.final_mass
            if len(acc) >= 2:
                got[acc[0], acc[1]] += pr
            elif len(acc) == 1:
                got[acc[0]] += pr * last
            else:
                for a in range(V):
                    got[a] += pr * last[a] * norm((a,))
        assert abs(total - 1) < 1e-12
        assert np.abs(got - want).max() < 1e-12, (seed, np.abs(got - want).max())
    assert len(shapes) >= 2                              # the topology did depend on the context


# ---------------------------------------------------------------- Python helpers
def test_dynamic_tree_spec_shapes_and_truncation():
    from specdec_amd.tree import DynamicTreeSpec
    for L, W, c in [(1, 1, 1), (5, 8, 8), (4, 2, 2), (3, 3, 2), (32, 1, 1), (32, 8, 8)]:
        F, base = yref.shape(L, W, c)
        sp = DynamicTreeSpec(L, W, c, 1)
        assert sp.frontier == F and sp.base == base and sp.pool_size == base[-1]
    sp = DynamicTreeSpec(5, 8, 8, 64)
    assert sp.pool_size == 264 and sp.truncated(9) is sp
    t = sp.truncated(1)
    assert (t.levels, t.width, t.branch, t.num_nodes, t.pool_size) == (1, 8, 8, 8, 8)
    assert sp.truncated(2).num_nodes == 64 and sp.truncated(2).pool_size == 72
    for bad in [(0, 1, 1, 1), (33, 1, 1, 1), (1, 0, 1, 1), (1, 9, 1, 1), (1, 1, 0, 1), (1, 1, 9, 1), (1, 1, 1, 2), (5, 8, 8, 65),
                (2, 2, 2, 0)]:
        with pytest.raises(ValueError):
            DynamicTreeSpec(*bad)
    with pytest.raises(ValueError):
        sp.truncated(0)


def test_dynamic_attention_inputs_equal_token_trees():
    from specdec_amd.tree import TokenTree, dynamic_attention_inputs
    parents = [[-1, -1, 0, 0, 1], [-1] + list(range(31)), [-1] * 8, [(i - 1) // 2 for i in range(64)]]
    for parent in parents:
        tree = TokenTree(parent)
        anc = torch.tensor([[a - (1 << 64) if a >= 1 << 63 else a for a in yref.transitive_closure(parent)]])
        depth = torch.tensor([tree.node_depth], dtype=torch.int32)
        for prefix, dt in ((3, torch.float32), (1, torch.bfloat16)):
            mask, pos = dynamic_attention_inputs(anc, depth, prefix, dt)
            wm, wp = tree.attention_inputs(prefix, dt)
            assert mask.dtype == dt and torch.equal(mask, wm) and torch.equal(pos, wp)
    # two sequences, two topologies
    a = [yref.transitive_closure(p) for p in ([-1, 0, 1], [-1, -1, -1])]
    mask, pos = dynamic_attention_inputs(torch.tensor(a), torch.tensor([[1, 2, 3], [1, 1, 1]], dtype=torch.int32), 2)
    assert mask.shape == (2, 1, 5, 5) and pos.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 2, 2]]
    assert torch.equal(mask[0], TokenTree([-1, 0, 1]).attention_inputs(2)[0][0])
    assert torch.equal(mask[1], TokenTree([-1, -1, -1]).attention_inputs(2)[0][0])


def test_fake_implementations_give_shapes():
    import specdec_amd  # noqa: F401
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    pool = (m(3, 264, dt=torch.long), m(3, 264), m(3, 264, dt=torch.int32))
    outs = torch.ops.specdec.tree_grow(m(3, 8, 1000, dt=torch.bfloat16), 3, 8, 8, *pool, m(3, 8, dt=torch.int32))
    assert [tuple(o.shape) for o in outs] == [(3, 8)] * 3 + [(3,)]
    assert [o.dtype for o in outs] == [torch.long, torch.int32, torch.int32, torch.int32]
    outs = torch.ops.specdec.tree_grow(m(3, 1, 1000), 1, 2, 3, *pool, None)
    assert [tuple(o.shape) for o in outs] == [(3, 2)] * 3 + [(3,)]
    outs = torch.ops.specdec.tree_select(*pool, 64, 264)
    assert [tuple(o.shape) for o in outs] == [(3, 64)] * 5 + [(3,)]
    assert [o.dtype for o in outs] == [torch.long, torch.int32, torch.int32, torch.int32, torch.long, torch.int32]
    outs = torch.ops.specdec.verify_tree_dynamic(m(3, 65, 1000), m(3, 64, dt=torch.long), m(3, 64, dt=torch.int32), 5,
                                                 m(0, dt=torch.long), 1, 1.0, 0, 1.0, 7, 0, 0)
    assert [tuple(o.shape) for o in outs] == [(3,)] * 7 + [(3, 5)]


def test_the_loop_is_exported_and_refuses_user_processors():
    from specdec_amd import dynamic_tree_speculative_generate
    from specdec_amd.sampling import dynamic_tree_speculative_generate as again
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    assert again is dynamic_tree_speculative_generate

    class Mine(MultinomialProcessor):
        def _process(self, logits):
            return logits

    with pytest.raises(TypeError):
        dynamic_tree_speculative_generate([1, 2], None, None, logits_processor=Mine(1.0))


# ---------------------------------------------------------------- the GPU suite's cases exist
def test_every_grid_case_has_a_seed_without_a_close_boundary():
    """The GPU tests compare tokens, parents and pool indices exactly, so their inputs must keep every
    frontier and final-N boundary more than 1e-3 wide (or exactly tied): a condition on the inputs,
    checked here on the host for every listed shape with N(0, 3^2) logits."""
    import tree_dynamic_cases as yc
    grid = yc.grid()
    assert len(grid) == len(yc.VOCABS) * len(yc.SHAPES) * len(yc.LEVELS)
    for name, values, at in (("B", yc.BATCHES, 1), ("L", yc.LEVELS, 4), ("dtype", yc.DTYPES, 6),
                             ("layout", yc.LAYOUTS, 7)):
        for V in yc.VOCABS:
            assert {g[at] for g in grid if g[0] == V} == set(values), (name, V)
    assert {g[5] for g in grid} >= {1, 7, 64} and any(g[3] == g[0] for g in grid)      # every N; c = V
    seeds = []
    for g in grid:
        c = yc.case(*g[:7])
        assert not any(m.close for m in c.models)
        assert all(x > yref.CLOSE or x == 0 for m in c.models for x in m.gaps)
        seeds.append(c.seed)
    print(f"[tree-dynamic] grid seeds: {seeds}")
    for g in ((2049, 3, 8, 8, 2, 64, torch.bfloat16), (4097, 1, 2, 3, 5, 7, torch.float32)):
        assert not any(m.close for m in yc.case(*g, mask=True).models)
