"""CPU checks of the token-tree verify: the rule's losslessness by exact enumeration, the host
model (tests/tree_ref.py) against the multi-draft one on chains, TokenTree's validation and its
attention inputs against a stock LlamaForCausalLM, the ctypes mirror against the header, the argument
checks of sd_verify_tree, and the coverage of the GPU case grid (tests/test_gpu_tree.py runs exactly
tree_walk.grid())."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import multidraft_ref as mref
import tree_ref as tref
import tree_walk as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the rule is lossless
def _ctx_rows(V, seed):
    """Context-dependent p(. | ctx), q(. | ctx): fixed random distributions per context tuple."""
    cache = {}

    def rows(ctx):
        if ctx not in cache:
            rng = np.random.default_rng([seed, len(ctx)] + list(ctx))
            cache[ctx] = (rng.dirichlet(np.ones(V)), rng.dirichlet(np.ones(V)))
        return cache[ctx]
    return rows


@pytest.mark.parametrize("parent", [[-1, -1, 0, 0, 1], tw.chains(2, 2), tw.from_branching([3])],
                         ids=["five-nodes", "chains-2x2", "fan-3"])
def test_first_two_tokens_keep_the_target_joint_exactly(parent):
    """V = 3, context-dependent p and q, every draft assignment (weighted by the q it was drawn from)
    and every branch of the walk: the joint of the first two emitted tokens is the target's,
    p(a | ()) p(b | (a,)), to 1e-12.  Where the step emits one token only, the second is the next
    step's, which the same rule draws from p(. | (a,)) exactly."""
    V, N = 3, len(parent)
    rows = _ctx_rows(V, 5)
    joint = np.zeros((V, V))
    total = 0.0
    for tok in itertools.product(range(V), repeat=N):
        ctx = [()]
        for i in range(N):
            ctx.append(ctx[parent[i] + 1] + (tok[i],))
        P = np.stack([rows(c)[0] for c in ctx])
        Q = np.stack([rows(c)[1] for c in ctx])
        w = 1.0
        for i in range(N):
            w *= Q[parent[i] + 1][tok[i]]                  # children are iid draws from their parent slot's q
        for prob, o in tref.enumerate_outcomes(P, Q, np.array(tok), parent):
            acc = [tok[c] for c in o.path]
            x = o.weights / o.weights.sum()
            total += w * prob
            if len(acc) >= 2:
                joint[acc[0], acc[1]] += w * prob
            elif len(acc) == 1:
                joint[acc[0]] += w * prob * x
            else:
                for a in range(V):
                    joint[a] += w * prob * x[a] * rows((a,))[0]
    want = np.array([[rows(())[0][a] * rows((a,))[0][b] for b in range(V)] for a in range(V)])
    assert abs(total - 1.0) < 1e-12
    assert np.abs(joint - want).max() < 1e-12, np.abs(joint - want).max()


# ---------------------------------------------------------------- chains walk as the multi-draft model
@pytest.mark.parametrize("K,g", [(1, 4), (2, 3), (4, 2), (3, 4), (8, 2)])
def test_chains_walk_as_the_multidraft_model(K, g):
    """The K-chains tree (node d*K + k, parent i - K) on rows whose depth-0 tokens are pairwise
    distinct: n, exit kind, winner, rejects, the mass and the final weights of multidraft_ref.walk."""
    V, rng = 12, np.random.default_rng(K * 100 + g)
    done = 0
    while done < 80:
        P = rng.dirichlet(np.ones(V) * 0.7, size=(K, g + 1))
        Q = rng.dirichlet(np.ones(V) * 0.7, size=(K, g))
        P[:, 0], Q[:, 0] = P[0, 0], Q[0, 0]               # one context at depth 0
        tok = np.stack([rng.choice(V, size=K, replace=False)] + [rng.integers(0, V, K) for _ in range(g - 1)], 1)
        u = rng.random(K * g)
        m = mref.walk(P, Q, tok, lambda d, k, j, frac, slack: not (u[d * K + k] > frac))
        Pt, Qt = tref.chains_rows(P, Q)
        t = tref.walk(Pt, Qt, tok.T.reshape(-1), tw.chains(K, g), lambda c, j, frac, slack: not (u[c] > frac))
        assert (t.n, t.status, t.rejects) == (m.n, m.status, m.rejects)
        if m.n > 0:
            assert t.last_node % K == m.winner and t.last_node // K == m.n - 1
        assert (np.isnan(t.mass) and np.isnan(m.mass)) or t.mass == m.mass
        assert np.array_equal(t.weights, m.weights)
        done += 1


# ---------------------------------------------------------------- TokenTree
def test_token_tree_validation_and_constructors():
    from specdec_amd.tree import TokenTree
    t = TokenTree([-1, -1, 0, 0, 1])
    assert (t.num_nodes, t.depth, t.max_children) == (5, 2, 2)
    assert t.children == [[0, 1], [2, 3], [4], [], [], []] and t.internal_slots == [0, 1, 2]
    assert t.levels == [[0, 1], [2, 3, 4]] and t.path_to(4) == [1, 4]
    assert TokenTree.from_branching([4, 2, 1, 1]).parent == tw.from_branching([4, 2, 1, 1])
    assert TokenTree.from_branching([4, 2, 1, 1]).num_nodes == 28
    assert TokenTree.chains(3, 4).parent == tw.chains(3, 4) and TokenTree.chains(3, 4).depth == 4
    assert TokenTree.from_branching([2, 2, 1]).truncated(2).parent == tw.from_branching([2, 2])
    for bad in ([], [0], [-2], [-1, 1], [-1, 2], [-1] * 9, list(range(-1, 32)), [-1] * 8 + [0] * 8 + [1] * 8 * 7):
        with pytest.raises(ValueError):
            TokenTree(bad)
    assert TokenTree([-1] * 8).max_children == 8 and TokenTree(list(range(-1, 31))).depth == 32
    assert TokenTree(tw.TREES["irregular64"]).num_nodes == 64
    mask, pos = t.attention_inputs(3, torch.float64)
    assert mask.shape == (1, 1, 8, 8) and pos.tolist() == [[0, 1, 2, 3, 3, 4, 4, 4]]
    allow = mask[0, 0] == 0
    assert allow[:3, :3].equal(torch.ones(3, 3).tril().bool()) and allow[3:, :3].all() and not allow[:3, 3:].any()
    assert allow[3:, 3:].int().tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 0, 0, 1, 0], [0, 1, 0, 0, 1]]
    assert float(mask.min()) == torch.finfo(torch.float64).min


def test_tree_attention_inputs_reproduce_the_plain_forward_of_every_path():
    """A random-init fp64 LlamaForCausalLM (2 layers, hidden 32, vocab 97) under the tree's 4-D additive
    mask and position_ids: every node's logits equal the plain forward on prefix + its path within 1e-9
    (fp64 rounding over a few thousand operations is far below that; a wrong mask moves logits by about
    1e-2), and the plain causal mask over the same tokens differs by more than 1e-3."""
    transformers = pytest.importorskip("transformers")
    from specdec_amd.tree import TokenTree
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=97, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64)
    tree = TokenTree([-1, -1, 0, 0, 1, 2, 2, 4])
    prefix = torch.tensor([[5, 17, 33, 2, 60]])
    nodes = torch.tensor([[11, 12, 13, 14, 15, 16, 17, 18]])
    ids = torch.cat([prefix, nodes], 1)
    worst = {}
    for impl in ("eager", "sdpa"):
        cfg._attn_implementation = impl
        try:
            model = transformers.LlamaForCausalLM(cfg).double().eval()
            mask, pos = tree.attention_inputs(prefix.shape[1], torch.float64)
            with torch.no_grad():
                got = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits[0]
                causal = model(input_ids=ids).logits[0]
        except (TypeError, ValueError, RuntimeError) as e:       # an installed version that refuses 4-D masks
            pytest.skip(f"transformers {transformers.__version__} rejects the 4-D additive mask: {e}")
        err = moved = 0.0
        for i in range(tree.num_nodes):
            path = tree.path_to(i)
            with torch.no_grad():
                plain = model(input_ids=torch.cat([prefix, nodes[:, path]], 1)).logits[0, -1]
            err = max(err, float((got[prefix.shape[1] + i] - plain).abs().max()))
            moved = max(moved, float((causal[prefix.shape[1] + i] - plain).abs().max()))
        with torch.no_grad():                                    # the prefix rows are the plain prefix forward's
            err = max(err, float((got[:prefix.shape[1]] - model(input_ids=prefix).logits[0]).abs().max()))
        worst[impl] = (err, moved)
        print(f"[tree-attn] {impl}: tree mask err={err:.3g}, causal mask moves logits by {moved:.3g}")
        assert err < 1e-9 and moved > 1e-3, (impl, err, moved)


# ---------------------------------------------------------------- struct layout, constants, exports
def test_tree_args_ctypes_layout_matches_the_header():
    from specdec_amd import _lib
    s = "sd_tree_args"
    old = ["sd_verify_args", "sd_sample_args", "sd_ngram_args", "sd_beam_args", "sd_multi_args", "sd_vp_args"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
    prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
    for f, _ in _lib.sd_tree_args._fields_:
        prog += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    for o in old:
        prog += f'  printf("{o}.size %zu\\n", sizeof({o}));\n'
    prog += ('  printf("limits %d %d %d %d %d\\n", SD_TREE_MAX_NODES, SD_TREE_MAX_CHILDREN, SD_TREE_MAX_BATCH, SD_MAX_GAMMA,'
             ' (int)SD_PATH_VERIFY_TREE);\n  printf("abi %d\\n", SD_ABI_VERSION);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got[f"{s}.size"]) == C.sizeof(_lib.sd_tree_args)
    for f, _ in _lib.sd_tree_args._fields_:
        assert getattr(_lib.sd_tree_args, f).offset == int(got[f"{s}.{f}"]), f
    assert got["limits"].split() == ["64", "8", "16384", "32", "8"]
    assert (_lib.SD_TREE_MAX_NODES, _lib.SD_TREE_MAX_CHILDREN, _lib.SD_TREE_MAX_BATCH, _lib.SD_PATH_VERIFY_TREE) == (64, 8, 16384, 8)
    assert got["abi"] == "12" and _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12
    for o in old:                                        # additive: the existing structs keep their sizes
        assert int(got[f"{o}.size"]) == C.sizeof(getattr(_lib, o)), o
    assert int(got["sd_multi_args.size"]) == 816 and int(got["sd_verify_args.size"]) == 888
    for name in ("sd_verify_tree", "sd_verify_tree_workspace_size"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.PATH_NAMES[_lib.SD_PATH_VERIFY_TREE] == "k_stats+k_tree_mass+k_tree_walk"


def _parent_array(parent):
    from specdec_amd import _lib
    return (C.c_int32 * _lib.SD_TREE_MAX_NODES)(*parent)


def test_workspace_size_and_argument_checks():
    """sd_verify_tree_workspace_size over topologies and the status of refused calls (no launch: every
    call here is refused before one)."""
    from specdec_amd import _lib
    lib = _lib.lib
    size = lambda B, parent, V, n=None: lib.sd_verify_tree_workspace_size(  # noqa: E731
        B, len(parent) if n is None else n, _parent_array(parent[:64]), V)
    good = tw.from_branching([4, 2, 1, 1])
    assert size(1, good, 4096) > 0 and size(1, good, 4096) % 256 == 0
    assert size(33, good, 4096) > size(1, good, 4096) and size(1, good, 128256) > size(1, good, 4096)
    assert size(0, good, 4096) == 0 and size(1, good, 0) == 0 and size(1, good, 4096, n=0) == 0
    assert size(1, [-1] * 64, 4096, n=65) == 0 and size(1, [-1, 1], 4096) == 0 and size(1, [-1, 0, 2], 4096) == 0
    assert size(1, [-2], 4096) == 0 and size(1, [-1] * 9, 4096) == 0 and size(1, list(range(-1, 32)), 4096) == 0
    assert size(1, [-1] * 8, 4096) > 0 and size(1, list(range(-1, 31)), 4096) > 0
    assert size(16384, tw.TREES["irregular64"], 128256) == 0      # a mass grid the runtime would refuse
    assert size(16385, [-1], 64) == 0
    assert lib.sd_verify_tree_workspace_size(1, 4, None, 4096) == 0

    def args(parent, **kw):
        a = _lib.sd_tree_args()
        a.batch, a.num_nodes, a.vocab = 2, len(parent), 4096
        a.parent = _parent_array(parent[:64])
        for s in range(min(len(parent), 64) + 1):
            a.target_rows[s] = 0x1000 + 64 * s
            a.draft_rows[s] = 0x9000 + 64 * s
        a.target_stride_b = a.draft_stride_b = 4096
        a.dtype = _lib.SD_BF16
        a.draft_tokens, a.draft_tokens_stride_b = 0x20000, 64
        a.proc = _lib.sd_processor(_lib.SD_PROC_MULTINOMIAL, 1.0, 0, 1.0)
        a.noise.mode, a.noise.seed = _lib.SD_NOISE_PHILOX, 7
        for i, f in enumerate(("n_accepted", "last_node", "next_token", "row_status", "path")):
            setattr(a, f, 0x30000 + 0x1000 * i)
        a.path_stride_b = 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.sd_verify_tree(C.byref(a), None)  # noqa: E731
    INV, UNS, WS = _lib.SD_ERR_INVALID, _lib.SD_ERR_UNSUPPORTED, _lib.SD_ERR_WORKSPACE
    assert lib.sd_verify_tree(None, None) == INV
    assert call(args(good)) == WS                                    # everything valid but the workspace
    assert call(args(good, workspace=0x40000, workspace_bytes=size(2, good, 4096) - 1)) == WS
    assert call(args(good, num_nodes=0)) == INV and call(args([-1] * 64, num_nodes=65)) == UNS
    assert call(args([-1, 1])) == INV and call(args([-1, 0, 2])) == INV and call(args([-3])) == INV
    assert call(args([-1] * 9)) == UNS and call(args(list(range(-1, 32)))) == UNS
    assert call(args(good, batch=0)) == INV and call(args(good, vocab=0)) == INV
    assert call(args(good, batch=16385)) == UNS
    for f in ("draft_tokens", "n_accepted", "last_node", "next_token", "row_status", "path"):
        assert call(args(good, **{f: None})) == INV, f
    a = args(good)
    a.target_rows[28] = None
    assert call(a) == INV
    a = args(good)
    a.draft_rows[0] = None                                           # the root has children
    assert call(a) == INV
    a = args(good)
    a.draft_rows[28] = None                                          # a leaf slot's drafter row may be null
    assert call(a) == WS
    assert call(args(good, n_stop=2)) == INV and call(args(good, n_stop=-1)) == INV
    assert call(args(good, path_stride_b=3)) == INV and call(args(good, draft_tokens_stride_b=27)) == INV
    assert call(args(good, tokens_out=0x50000, tokens_out_stride_b=4)) == INV
    assert call(args(good, dtype=9)) == INV
    a = args(good)
    a.noise.mode = _lib.SD_NOISE_STREAM
    assert call(a) == UNS
    a.noise.mode = 5
    assert call(a) == INV
    a = args(good)
    a.proc.temperature = 0.0
    assert call(a) == INV


def test_ops_verify_tree_refuses_what_verify_multi_refuses():
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise, StreamNoise
    from specdec_amd.utils.logits_processor import MultinomialProcessor

    class Mine(MultinomialProcessor):
        def _process(self, logits):
            return logits

    t = torch.zeros(1, 2, 8)
    tok = torch.zeros(1, 1, dtype=torch.long)
    spec = ops.ProcSpec("multinomial", 1.0)
    with pytest.raises(TypeError):
        ops.verify_tree(t, t[:, :1], tok, [-1], spec, StreamNoise(torch.Generator()))
    with pytest.raises(TypeError):
        ops.verify_tree(t, t[:, :1], tok, [-1], Mine(1.0), PhiloxNoise(seed=1))
    with pytest.raises(ValueError):
        ops.verify_tree(t, t[:, :1], tok, [-1, 1], spec, PhiloxNoise(seed=1))          # bad topology
    with pytest.raises(ValueError):
        ops.verify_tree(torch.zeros(1, 3, 8), t[:, :1], tok, [-1], spec, PhiloxNoise(seed=1))   # N+1 target rows
    with pytest.raises(ValueError):
        ops.verify_tree(t, t, tok, [-1], spec, PhiloxNoise(seed=1))                    # one internal slot, two rows
    with pytest.raises(ValueError):
        ops.verify_tree(t, t[:, :1], tok, [-1], spec, PhiloxNoise(seed=1))             # host tensors


def test_verify_tree_op_fake_shapes():
    import specdec_amd  # noqa: F401
    parent = tw.from_branching([2, 2, 1])
    with torch._subclasses.FakeTensorMode():
        target = torch.empty(3, len(parent) + 1, 64, dtype=torch.bfloat16)
        draft = torch.empty(3, 7, 64, dtype=torch.bfloat16)
        tok = torch.empty(3, len(parent), dtype=torch.long)
        out = torch.ops.specdec.verify_tree(target, draft, tok, parent, torch.empty(0, dtype=torch.long), 1, 1.0, 0, 1.0,
                                            1, 0, 0)
    assert [tuple(o.shape) for o in out] == [(3,)] * 7 + [(3, 3)]
    assert out[2].dtype == torch.long and out[3].dtype == torch.float32 and out[7].dtype == torch.int32


# ---------------------------------------------------------------- coverage of the GPU grid
@pytest.fixture(scope="module")
def grid_coverage():
    out = []
    for case in tw.grid():
        c = tw.case(*case)
        out.append((case, tw.coverage(c, tw.host_results(c)), tw.feasible(c.parent, c.V)))
    return out


def test_gpu_grid_holds_the_issue_shapes():
    g = tw.grid()
    assert {c[0] for c in g} == {1, 33} and {c[2] for c in g} == set(tw.VOCABS) == {1, 2, 3, 64, 2047, 2048, 2049, 4097, 50257}
    assert {c[1] for c in g} == set(tw.TREES) and {c[3] for c in g} == set(tw.DTYPES)
    assert {tw.PROCS[c[4]].kind for c in g} == {"greedy", "multinomial", "topk", "nucleus", "topknucleus"}
    for tname in tw.TREES:
        mine = [c for c in g if c[1] == tname]
        assert {c[0] for c in mine} == {1, 33} and {c[3] for c in mine} == set(tw.DTYPES), tname
    assert (len(tw.TREES["one"]), len(tw.TREES["chain32"]), len(tw.TREES["irregular64"])) == (1, 32, 64)
    assert all(c[5] for c in g if c[2] in (2049, 4097)) and not any(c[5] for c in g if c[2] <= 2048)


def test_gpu_cases_reach_every_branch(grid_coverage):
    """Every case from V = 64 up (below it the steering has no tokens to choose from: V = 1 accepts
    everything, V <= 3 must only show both exit kinds over the grid) finds, where its tree allows it,
    residual exits at the root and below, bonus exits at leaves of at least two depths, a slot with at
    least two rejected siblings and, where V has a second chunk, a draw in it."""
    tiny_resid = tiny_bonus = 0
    for case, cov, can in grid_coverage:
        print(case[:5], vars(cov))
        if case[2] < 64:
            tiny_resid += cov.resid_root + cov.resid_deep
            tiny_bonus += len(cov.bonus_depths) > 0
            continue
        assert cov.resid_root >= 1, case
        assert cov.resid_deep >= 1 or not can.resid_deep, case
        assert len(cov.bonus_depths) >= min(2, can.bonus_depths), case
        assert cov.two_rejects >= 1 or not can.two_rejects, case
        assert cov.late_chunk >= 1 or not can.late_chunk, case
    assert tiny_resid >= 3 and tiny_bonus >= 10


def test_no_gpu_case_has_more_than_one_close_row(grid_coverage):
    for case, cov, _ in grid_coverage:
        assert cov.close <= 1, (case, cov.close)


def test_the_gpu_tests_other_cases_are_not_close():
    """The cases tests/test_gpu_tree.py runs outside the grid (stop lists, capture, layouts) hold at
    most one close row each too."""
    for args in [(33, "b4211", 2049, torch.bfloat16, "multinomial", True), (1, "irregular64", 64, torch.float32, "topk50"),
                 (33, "fan8", 4097, torch.float16, "multinomial_T0.7", True),
                 (33, "b4211", 2047, torch.bfloat16, "multinomial", False, "none"), (33, "b4211", 65, torch.float32, "topk50", False, "half"),
                 (33, "b4211", 2049, torch.float16, "greedy", False, "half"), (33, "b4211", 9, torch.bfloat16, "nucleus0.9", False, "most")]:
        c = tw.case(*args)
        assert sum(r.close for r in tw.host_results(c)) <= 1, args
    c = tw.case(33, "b4211", 2049, torch.bfloat16, "multinomial", True)
    assert sum(r.close for r in tw.host_results(c, off=1 + tw.OFFSET + 5)) <= 1       # the captured replay's offset
    assert sum(r.n >= 2 for r in tw.host_results(c)) >= 1                             # the stop test's row exists
