"""CPU checks of the token-tree verify for distinct children (sd_verify_tree_distinct): the rule's
losslessness by exact enumeration on the host model (tests/tree_distinct_ref.py), greedy against the
target's own greedy continuation, the ctypes mirror against the header, and the status of refused
calls (no launch: every call here is refused before one)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tree_distinct_ref as dref
import tree_walk as tw
from tree_ref import children_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4
TREES = {"five-nodes": [-1, -1, 0, 0, 1], "fan-3": tw.from_branching([3]), "two-two": tw.from_branching([2, 2])}
# how the children's tokens depart from the drafter's top-c: "dup" repeats the first child's token at the
# second child of the root, "oob" puts an id outside [0, V) there (alternating -1 and V by seed)
VARIANTS = ("top", "dup", "oob")


def _ctx_rows(seed, unique_max=False):
    """Context-dependent rows: p(. | ctx) unnormalised (Z != 1, as rounded probabilities are), the
    drafter's q(. | ctx) and the logits y(. | ctx) with p = exp(y), fixed per context tuple."""
    cache = {}

    def rows(ctx):
        if ctx not in cache:
            rng = np.random.default_rng([seed, len(ctx)] + [int(t) + 2 for t in ctx])
            y = rng.normal(size=V) * 1.5
            if unique_max:
                assert np.sum(y == y.max()) == 1
            cache[ctx] = (np.exp(y) * rng.uniform(0.9, 1.1), rng.dirichlet(np.ones(V)), y)
        return cache[ctx]
    return rows


def _tree_rows(parent, rows, variant, seed):
    """(P [N+1, V], Y [N+1, V], tok [N], ctx by slot): the children of a slot are the top-c tokens of
    q(. | the slot's context), a deterministic function of the context, then the variant's edit."""
    N, ch = len(parent), children_of(parent)
    ctx, tok = [()] + [None] * N, [0] * N
    for s in range(N + 1):
        if not ch[s]:
            continue
        best = dref.topk_tokens(rows(ctx[s])[1], len(ch[s]))
        for j, c in enumerate(ch[s]):
            tok[c] = best[j]
            if s == 0 and j == 1 and variant == "dup":
                tok[c] = best[0]
            if s == 0 and j == 1 and variant == "oob":
                tok[c] = -1 if seed % 2 else V
            ctx[c + 1] = ctx[s] + (tok[c],)
    P = np.stack([rows(c)[0] for c in ctx])
    Y = np.stack([rows(c)[2] for c in ctx])
    return P, Y, np.array(tok), ctx


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tname", list(TREES))
def test_first_two_tokens_keep_the_target_joint_exactly(tname, variant):
    """V = 4, context-dependent p, children the top-c of a context-dependent q (one variant forces a
    duplicate sibling, one an out-of-range id), every branch of the walk with its exact probability:
    the joint of the first two emitted tokens is the target's, to 1e-12.  A step that emits one token
    leaves the second to the next step, which emits p(. | first) by the same argument."""
    parent = TREES[tname]
    for seed in range(6):
        rows = _ctx_rows(seed)
        P, _, tok, _ = _tree_rows(parent, rows, variant, seed)
        norm = lambda ctx: rows(ctx)[0] / rows(ctx)[0].sum()  # noqa: E731
        want = np.array([[norm(())[a] * norm((a,))[b] for b in range(V)] for a in range(V)])
        got, total, seen = np.zeros((V, V)), 0.0, set()
        for pr, o in dref.enumerate_outcomes(P, tok, parent):
            total += pr
            seen.add((o.status, o.n))
            acc = [int(tok[c]) for c in o.path]
            last = o.weights / o.final_mass
            if len(acc) >= 2:
                got[acc[0], acc[1]] += pr
            elif len(acc) == 1:
                got[acc[0]] += pr * last
            else:
                for a in range(V):
                    got[a] += pr * last[a] * norm((a,))
        assert abs(total - 1) < 1e-12
        assert np.abs(got - want).max() < 1e-12, (tname, variant, seed, np.abs(got - want).max())
        assert (dref.RESIDUAL, 0) in seen and any(n >= 1 for _, n in seen)
        if variant != "top":                     # the edited child has no weight: never accepted, never asked
            assert all(c != children_of(parent)[0][1] for _, o in dref.enumerate_outcomes(P, tok, parent)
                       for c, _, _, _ in o.tests)


def test_the_slot_accepts_with_the_mass_of_its_children():
    """Total acceptance at a slot is p(C) / Z, whatever the order of the children."""
    rows = _ctx_rows(3)
    p = rows(())[0]
    for toks in ([2, 0, 3], [3, 2, 0], [1]):
        parent = [-1] * len(toks)
        P = np.stack([p] + [rows((t,))[0] for t in toks])
        acc = sum(pr for pr, o in dref.enumerate_outcomes(P, np.array(toks), parent) if o.n == 1)
        assert abs(acc - p[toks].sum() / p.sum()) < 1e-12


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tname", list(TREES))
def test_greedy_emits_the_targets_greedy_continuation(tname, variant):
    """Rows with unique maxima: the emitted tokens are the target's greedy continuation along the
    tree, and the walk accepts exactly as deep as the drafted children follow it."""
    parent = TREES[tname]
    depths = set()
    for seed in range(200):
        rows = _ctx_rows(seed, unique_max=True)
        P, Y, tok, ctx = _tree_rows(parent, rows, variant, seed)
        r = dref.philox_step(P, tok, parent, 1234, 5, 0, Y=Y)
        want, c = [], ()
        for _ in range(r.n + 1):
            want.append(int(np.argmax(rows(c)[2])))
            c = c + (want[-1],)
        assert r.emitted == want, (seed, r.emitted, want)
        # no deeper path existed: the greedy token after the emitted ones is no child of the exit slot
        assert want[-1] not in [int(tok[k]) for k in children_of(parent)[r.slot]]
        assert ctx[r.slot] == tuple(want[:-1])
        depths.add(r.n)
    assert len(depths) >= 2


def test_philox_step_flags_close_tests_and_scans_stops():
    parent = TREES["two-two"]
    rows = _ctx_rows(1)
    P, _, tok, _ = _tree_rows(parent, rows, "top", 1)
    hit = next(r for r in (dref.philox_step(P, tok, parent, 77, off, 0) for off in range(64)) if r.n >= 1)
    assert hit.stop_index == -1 and hit.x is not None and hit.lo <= hit.u * hit.total < hit.hi
    off = next(o for o in range(64) if dref.philox_step(P, tok, parent, 77, o, 0).n >= 1)
    stopped = dref.philox_step(P, tok, parent, 77, off, 0, stops=[hit.accepted[0]])
    assert stopped.status == dref.STOP and stopped.stop_index == 0 and stopped.x is None
    assert not hit.close


# ---------------------------------------------------------------- struct layout, constants, exports
def test_tree_distinct_args_ctypes_layout_matches_the_header():
    from specdec_amd import _lib
    s = "sd_tree_distinct_args"
    old = ["sd_verify_args", "sd_sample_args", "sd_ngram_args", "sd_beam_args", "sd_multi_args", "sd_vp_args", "sd_tree_args",
           "sd_kv_compact_args"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
    prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
    for f, _ in _lib.sd_tree_distinct_args._fields_:
        prog += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    for o in old:
        prog += f'  printf("{o}.size %zu\\n", sizeof({o}));\n'
    prog += ('  printf("path %d\\n", (int)SD_PATH_VERIFY_TREE_DISTINCT);\n  printf("abi %d\\n", SD_ABI_VERSION);\n'
             '  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got[f"{s}.size"]) == C.sizeof(_lib.sd_tree_distinct_args)
    for f, _ in _lib.sd_tree_distinct_args._fields_:
        assert getattr(_lib.sd_tree_distinct_args, f).offset == int(got[f"{s}.{f}"]), f
    # sd_tree_args without draft_rows / draft_stride_b
    assert [f for f, _ in _lib.sd_tree_distinct_args._fields_] == [f for f, _ in _lib.sd_tree_args._fields_
                                                                   if f not in ("draft_rows", "draft_stride_b")]
    assert got["path"] == "9" and _lib.SD_PATH_VERIFY_TREE_DISTINCT == 9
    assert got["abi"] == "12" and _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12
    for o in old:                                        # additive: the existing structs keep their sizes
        assert int(got[f"{o}.size"]) == C.sizeof(getattr(_lib, o)), o
    for name in ("sd_verify_tree_distinct", "sd_verify_tree_distinct_workspace_size"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.PATH_NAMES[_lib.SD_PATH_VERIFY_TREE_DISTINCT] == "k_stats+k_treed_rowsum+k_treed_walk"


def _parent_array(parent):
    from specdec_amd import _lib
    return (C.c_int32 * _lib.SD_TREE_MAX_NODES)(*parent)


def test_workspace_size_and_argument_checks():
    from specdec_amd import _lib
    lib = _lib.lib
    size = lambda B, parent, V, n=None: lib.sd_verify_tree_distinct_workspace_size(  # noqa: E731
        B, len(parent) if n is None else n, _parent_array(parent[:64]), V)
    good = tw.from_branching([4, 2, 1, 1])
    assert size(1, good, 4096) > 0 and size(1, good, 4096) % 256 == 0
    assert size(33, good, 4096) > size(1, good, 4096) and size(1, good, 128256) > size(1, good, 4096)
    # no drafter rows, no mass tables: never more than sd_verify_tree asks for
    assert size(33, good, 128256) < lib.sd_verify_tree_workspace_size(33, len(good), _parent_array(good), 128256)
    assert size(0, good, 4096) == 0 and size(1, good, 0) == 0 and size(1, good, 4096, n=0) == 0
    assert size(1, [-1] * 64, 4096, n=65) == 0 and size(1, [-1, 1], 4096) == 0 and size(1, [-2], 4096) == 0
    assert size(1, [-1] * 9, 4096) == 0 and size(1, list(range(-1, 32)), 4096) == 0
    assert size(1, [-1] * 8, 4096) > 0 and size(1, list(range(-1, 31)), 4096) > 0
    assert size(16385, [-1], 64) == 0
    assert lib.sd_verify_tree_distinct_workspace_size(1, 4, None, 4096) == 0

    def args(parent, **kw):
        a = _lib.sd_tree_distinct_args()
        a.batch, a.num_nodes, a.vocab = 2, len(parent), 4096
        a.parent = _parent_array(parent[:64])
        for s in range(min(len(parent), 64) + 1):
            a.target_rows[s] = 0x1000 + 64 * s
        a.target_stride_b = 4096
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

    call = lambda a: lib.sd_verify_tree_distinct(C.byref(a), None)  # noqa: E731
    INV, UNS, WS = _lib.SD_ERR_INVALID, _lib.SD_ERR_UNSUPPORTED, _lib.SD_ERR_WORKSPACE
    assert lib.sd_verify_tree_distinct(None, None) == INV
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
    assert call(args(good, path_stride_b=3)) == INV and call(args(good, draft_tokens_stride_b=27)) == INV
    assert call(args(good, n_stop=2)) == INV
    a = args(good)
    a.noise.mode = _lib.SD_NOISE_STREAM
    assert call(a) == UNS
    a.noise.mode = 5
    assert call(a) == INV


def test_loop_rejects_an_unknown_children_mode():
    from specdec_amd.sampling import tree_speculative_generate
    with pytest.raises(ValueError, match="children"):
        tree_speculative_generate([1, 2], None, None, children="beam")
