"""CPU checks of the multi-draft verify: the rule itself (exact enumeration against the target's
distribution), the host model against the single-chain host walk, the coverage of the GPU cases
(tests/test_gpu_multidraft.py runs multi_walk.grid() and edge_grid(), tests/test_gpu_multidraft_edges.py
small_grid()) and the sharpness of their draw check, the C ABI's argument checks through ctypes, and
the torch op's fake implementation."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import multi_walk as mw
import multidraft_ref as mref
import perf_walk
import row_edges as rowe


# ---------------------------------------------------------------- the rule is lossless
def _ctx_rows(V, seed):
    """Context-dependent p and q: a distribution per prefix of length 0, 1 and 2."""
    def dist(prefix, which):
        r = np.random.default_rng([seed, which, len(prefix)] + list(prefix))
        v = r.random(V) + 0.05
        return v / v.sum()

    return (lambda pre: dist(pre, 0)), (lambda pre: dist(pre, 1))


@pytest.mark.parametrize("K", [1, 2, 3])
def test_exact_enumeration_reproduces_the_target_joint(K):
    """V = 3, γ = 2: over every draft assignment (weighted by its probability under q) and every
    accept / reject branch, the joint of the first two emitted tokens equals the target's to 1e-12.
    A step that emitted one token is extended by the target's next row."""
    V, g = 3, 2
    p_of, q_of = _ctx_rows(V, 41)
    joint = np.zeros((V, V))
    chain_toks = list(itertools.product(range(V), repeat=g))
    for combo in itertools.product(chain_toks, repeat=K):
        tok = np.array(combo)                                    # [K, γ]
        pr_tok = 1.0
        for k in range(K):
            for d in range(g):
                pr_tok *= q_of(list(tok[k, :d]))[tok[k, d]]
        P = np.array([[p_of(list(tok[k, :d])) for d in range(g + 1)] for k in range(K)])
        Q = np.array([[q_of(list(tok[k, :d])) for d in range(g)] for k in range(K)])
        for pr, o in mref.enumerate_outcomes(P, Q, tok):
            w = o.weights / o.weights.sum()
            acc = [int(t) for t in tok[o.winner, :o.n]]
            if o.n == 2:
                joint[acc[0], acc[1]] += pr_tok * pr
            elif o.n == 1:
                joint[acc[0], :] += pr_tok * pr * w
            else:
                for x in range(V):
                    joint[x, :] += pr_tok * pr * w[x] * p_of([x])
    want = np.array([[p_of([])[a] * p_of([a])[b] for b in range(V)] for a in range(V)])
    assert abs(joint.sum() - 1) < 1e-12
    assert np.abs(joint - want).max() < 1e-12, np.abs(joint - want).max()


def test_a_rejected_token_is_never_accepted_from_a_sibling():
    """Why no case re-admits an earlier-rejected chain: a test of token x fails only when
    r[x] / q[x] < u < 1, so r[x] < q[x] and the next residual is 0 at x — a later sibling holding x
    is tested against 0 and fails for every u > 0.  The alive set's "same token" rule therefore only
    ever adds chains that were not yet tried (which the GPU cases cover: coverage().kept_untried)."""
    V, K = 3, 3
    p_of, q_of = _ctx_rows(V, 43)
    P = np.array([[p_of([]), p_of([0])]] * K)
    Q = np.array([[q_of([])]] * K)
    for x in range(V):
        tok = np.full((K, 1), x)
        for pr, o in mref.enumerate_outcomes(P, Q, tok):
            assert not o.readmit
            failed = False
            for d, k, j, frac, acc in o.tests:
                assert not failed or (frac == 0.0 and not acc)
                failed |= not acc


def test_pair_distribution_formula_equals_the_enumeration():
    """multi_walk.pair_distribution (the GPU pair test's reference) against the enumeration over
    drafts and branches at V = 4, K = 1..3, context-free rows."""
    V = 4
    p_of, q_of = _ctx_rows(V, 47)
    p0, q0, p1, q1, pb = p_of([]), q_of([]), p_of([9]), q_of([9]), p_of([9, 9])
    for K in (1, 2, 3):
        got = np.zeros((V, V))
        P = np.broadcast_to(np.array([p0, p1, pb]), (K, 3, V))
        Q = np.broadcast_to(np.array([q0, q1]), (K, 2, V))
        for combo in itertools.product(itertools.product(range(V), repeat=2), repeat=K):
            tok = np.array(combo)
            pr_tok = np.prod([q0[tok[k, 0]] * q1[tok[k, 1]] for k in range(K)])
            for pr, o in mref.enumerate_outcomes(P, Q, tok):
                if o.n == 2:
                    got[tok[o.winner, 0], tok[o.winner, 1]] += pr_tok * pr
                elif o.n == 1:
                    got[tok[o.winner, 0], :] += pr_tok * pr * o.weights / o.weights.sum()
        w0, w1 = mw.pair_distribution(p0, q0, p1, K)
        assert np.abs(got - np.outer(w0, w1)).max() < 1e-12


# ---------------------------------------------------------------- K = 1 is the single-chain walk
def test_one_chain_walk_equals_host_walk_spec():
    c = perf_walk.walk_case("long", 200, 4, 512, torch.bfloat16, 3)
    seed, off = 0xABCDEF, 2
    for b in range(c.B):
        P, Q = c.P[b].double().numpy()[None], c.Q[b].double().numpy()[None]
        r = mref.philox_step(P, Q, c.ids[b].numpy()[None], seed, off, b)
        p = [float(c.P[b, i, c.ids[b, i]]) for i in range(4)]
        q = [float(c.Q[b, i, c.ids[b, i]]) for i in range(4)]
        n, close = perf_walk.host_walk_spec(p, q, seed, off, b, 4)
        assert r.n == n and r.winner == 0 and r.rejects == (n < 4)
        assert not r.close or close


# ---------------------------------------------------------------- coverage of the GPU cases
@pytest.mark.parametrize("case", [c for c in mw.grid() if c[0] == 16],
                         ids=lambda c: f"K{c[1]}-g{c[2]}-V{c[3]}-{c[5]}")
def test_gpu_cases_reach_every_branch(case):
    """Every (K, γ) of the GPU walk grid has one 16-sequence case; it must contain each branch its
    shape can reach: an accept of a non-first sibling at depth >= 1 (K >= 2, γ >= 2), an all-rejected
    exit at depth 0 and one at depth >= 1 (γ >= 2), a full accept with winner != 0 (K >= 2), accept
    tests at uniform indices d*K + k in Philox blocks >= 1 (K γ > 4) — and at most one close
    sequence.  (The 1- and 3-sequence cases of the grid run other grid shapes of the launches.)  An
    alive set that re-admits an earlier-rejected chain cannot occur (see the test above); the host
    model reports none."""
    c = mw.case(*case)
    cov = mw.coverage(c, mw.host_results(c))
    f = mw.feasible(c.K, c.gamma)
    assert cov.rej0 >= 1 and cov.full >= 1
    assert cov.sib_deep >= 1 or not f.sib_deep
    assert cov.rej_deep >= 1 or not f.rej_deep
    assert cov.full_other >= 1 or not f.full_other
    assert cov.kept_untried >= 1 or c.K < 2
    assert cov.blocks >= 1 or not f.blocks
    assert cov.readmit == 0
    assert cov.close <= 1


def test_other_gpu_cases_have_at_most_one_close_sequence():
    """The 1- and 3-sequence cases of the grid, the V = 128256 one included."""
    for case in mw.grid():
        if case[0] != 16:
            c = mw.case(*case)
            assert sum(r.close for r in mw.host_results(c)) <= 1, case


# ---------------------------------------------------------------- the draw check of the GPU cases
def _gpu_case(kind, case):
    if kind == "edge":
        return mw.edge_case(*case)
    return mw.small_case(*case[:7]) if kind == "small" else mw.case(*case)


# what the GPU files run: the walk grid, the stop-list test's case, the chunk edges, the small vocabularies
DRAW_CASES = ([("grid", c) for c in mw.grid()] + [("grid", (16, 4, 4, 4096, torch.bfloat16, "multinomial"))]
              + [("edge", c) for c in mw.edge_grid()] + [("small", c) for c in mw.small_grid()])


def _case_id(kc):
    return kc[0] + "-" + "-".join(str(v).split(".")[-1] for v in kc[1])


@pytest.mark.parametrize("kc", DRAW_CASES, ids=_case_id)
def test_draw_check_is_sharp_on_every_gpu_case(kc):
    """The GPU check holds the device's token to the host's target u·Σ within 2·slack of the token's
    running-total interval.  That says something only while the interval is wider than what it is
    widened by: 4·slack < w[x] in at least 90 % of a case's drawn rows; and the widening admits a
    neighbouring token in at most 2 rows of a case (host target within 2·slack of lo or hi)."""
    c = _gpu_case(*kc)
    m = mw.draw_margins(c, mw.host_results(c))
    wide = [b for b, slack, w, edge in m if 4 * slack < w]
    near = [b for b, slack, w, edge in m if edge <= 2 * slack]
    if m:
        print(f"[draw-margin] {_case_id(kc)} drawn={len(m)} wide={len(wide)} near={near} "
              f"worst 2 slack / w[x]={max(2 * slack / w for b, slack, w, edge in m):.3g}")
    assert len(wide) >= 0.9 * len(m), (len(wide), len(m))
    assert len(near) <= 2, near


def test_edge_cases_draw_on_both_sides_of_the_last_chunk():
    """The boosted-tail cases of multi_walk.edge_grid() on the host model: each has at least 3 rows
    whose token lies in the short last chunk and at least 3 in an earlier one, at most one close row,
    and (greedy) a maximum that is unique by the GPU check's 1e-4 margin, so the cross-chunk argmax
    is exact; over the set, both exits draw from the last chunk and a residual draw follows two or
    more rejections at its node.  Every case, boosted or not, has at most one close row."""
    exits, deep = set(), 0
    for case in mw.edge_grid():
        c = mw.edge_case(*case)
        rows = mw.host_results(c)
        assert sum(r.close for r in rows) <= 1, case
        if not c.proc.stochastic:
            assert all(int((r.weights >= r.weights.max() * (1 - 1e-4)).sum()) == 1 for r in rows), case
        if not c.tail:
            continue
        first = mw.last_chunk_start(c.V)
        assert 0 < c.V - first < mw.CHUNK and first >= mw.CHUNK
        last = [r for r in rows if r.x is not None and r.x >= first]
        assert len(last) >= 3 and sum(r.x is not None and r.x < first for r in rows) >= 3, (case, len(last))
        if c.proc.stochastic:
            exits |= {r.status for r in last}
            deep += sum(r.status == mref.RESIDUAL and len(r.masses) >= 2 for r in rows)
    assert exits == {mref.RESIDUAL, mref.BONUS}
    assert deep >= 1
    # plain rows never reach the last chunk: why the tail is boosted
    plain = [mw.edge_case(*case) for case in mw.edge_grid() if case[3] > mw.CHUNK and not case[6] and case[5] != "greedy"]
    assert plain and not any(r.x >= mw.last_chunk_start(c.V) for c in plain for r in mw.host_results(c))


def test_small_cases_on_the_host_model():
    """tests/test_gpu_multidraft_edges.py's cases: top-k with k > V is k = V (the keep is the whole
    finite row), V = 1 gives bonus exits only, every larger V reaches both exits in some case, no case
    has more than one close row, and building the cases warns of nothing (a zero residual sum at small
    V leaves the iid draft)."""
    import warnings
    from oracle import specdec_ref as ref
    exits = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for case in mw.small_grid():
            B, K, g, V, dtype, name, mask, layout, hinted = case
            c = mw.small_case.__wrapped__(*case[:7])
            rows = mw.host_results(c)
            assert sum(r.close for r in rows) <= 1, case
            exits.setdefault(V, set()).update(r.status for r in rows)
            if name == "topk50" and V < 50:
                all_of = ref.Processor("topk", 1.0, top_k=V)
                plain = ref.Processor("multinomial", 1.0)
                for x in (c.tl, c.dl):
                    assert torch.equal(ref.process(x, c.proc, exact=True), ref.process(x, all_of, exact=True))
                    assert torch.equal(ref.process(x, c.proc, exact=True), ref.process(x, plain, exact=True))
            # a target row and its drafter row have the same `-inf` entries
            assert torch.equal(c.tl[:, :, :g].isinf(), c.dl.isinf()), case
    assert exits[1] == {mref.BONUS}
    assert all(exits[V] == {mref.RESIDUAL, mref.BONUS} for V in mw.SMALL_VOCABS if V > 1), exits
    vs = {(c[3], c[7]) for c in mw.small_grid()} | {(c[3], c[4]) for c in mw.small_grid()}
    assert all((V, x) in vs for V in mw.SMALL_VOCABS for x in rowe.LAYOUTS + tuple(mw.DTYPES))
    assert len(mw.small_grid()) <= 150


# ---------------------------------------------------------------- C ABI argument checks (ctypes)
def test_verify_multi_rejects_bad_arguments_before_any_hip_call():
    from specdec_amd import _lib
    lib = _lib.lib
    assert lib.sd_verify_multi(None, None) == _lib.SD_ERR_INVALID
    a = _lib.sd_multi_args()
    a.batch, a.num_drafts, a.gamma, a.vocab = 1, 2, 4, 100
    a.proc = _lib.sd_processor(_lib.SD_PROC_MULTINOMIAL, 1.0, 0, 1.0)
    a.noise.mode = _lib.SD_NOISE_PHILOX
    assert lib.sd_verify_multi(C.byref(a), None) == _lib.SD_ERR_INVALID      # null pointers
    assert lib.sd_verify_multi_workspace_size(1, 2, 4, 100) > 0
    for shape in ((0, 2, 4, 100), (1, 0, 4, 100), (1, 9, 4, 100), (1, 2, 33, 100), (1, 8, 9, 100), (8193, 2, 4, 100),
                  (1, 2, 4, 0)):
        assert lib.sd_verify_multi_workspace_size(*shape) == 0, shape
    assert lib.sd_verify_multi_workspace_size(8192, 2, 4, 100) > 0
    assert lib.sd_verify_multi_workspace_size(1, 8, 8, 128256) > lib.sd_verify_workspace_size(8, 8, 128256)


# ---------------------------------------------------------------- torch op
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_verify_multi_op_fake_shapes(dtype):
    import specdec_amd  # noqa: F401  (registers the ops)
    B, K, g, V = 3, 4, 5, 128256
    t = torch.empty(B, K, g + 1, V, device="meta", dtype=dtype)
    d = torch.empty(B, K, g, V, device="meta", dtype=dtype)
    tok = torch.empty(B, K, g, device="meta", dtype=torch.long)
    stops = torch.empty(2, device="meta", dtype=torch.long)
    out = torch.ops.specdec.verify_multi(t, d, tok, stops, 1, 1.0, 0, 1.0, 7, 0, 0)
    assert len(out) == 9
    want = [torch.int32, torch.int32, torch.long, torch.float32] + [torch.int32] * 5
    for o, dt in zip(out, want):
        assert (o.shape, o.dtype, o.device.type) == ((B,), dt, "meta")


def test_loop_refuses_user_processors_and_bad_draft_counts():
    from specdec_amd.sampling import multidraft_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor

    class Own(MultinomialProcessor):
        def _process(self, logits):
            return logits

    class OwnSample(MultinomialProcessor):
        def sample(self, probs):
            return probs.argmax(-1)

    for proc in (Own(1.0), OwnSample(1.0)):
        with pytest.raises(TypeError):
            multidraft_speculative_generate([1, 2], None, None, logits_processor=proc)
    for k in (0, 9):
        with pytest.raises(ValueError):
            multidraft_speculative_generate([1, 2], None, None, num_drafts=k)


def test_four_drafts_gain_on_the_loop_tests_pair():
    """What the device loop's K = 4 >= K = 1 inequality rests on: on the GPU loop test's FakeLM pair
    (vocab 4096, sigma 1, multinomial, γ = 4) the host model accepts clearly more drafts per step with
    four chains than with one (about 1.89 against 1.49 over longer runs), far above 5 %."""
    import fakelm
    target, drafter = fakelm.make_pair(4096, sigma=1.0)
    one = sum(mw.simulate_acceptance(target, drafter, 1, 4, 150, s) for s in range(2)) / 2
    four = sum(mw.simulate_acceptance(target, drafter, 4, 4, 150, s) for s in range(2)) / 2
    print(f"accepted drafts per step: K=1 {one:.3f}, K=4 {four:.3f}")
    assert four >= 1.05 * one


def test_multi_args_ctypes_layout_matches_the_header():
    """sizeof and field offsets of sd_multi_args: the ctypes mirror against the C header (gcc)."""
    import os
    import subprocess
    import tempfile
    from specdec_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.sd_multi_args._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
            '  printf("size %zu\\n", sizeof(sd_multi_args));\n'
            + "".join(f'  printf("{f} %zu\\n", offsetof(sd_multi_args, {f}));\n' for f in fields)
            + '  printf("limits %d %d %d\\n", SD_MULTI_MAX_DRAFTS, SD_MULTI_MAX_NODES, SD_MULTI_MAX_ROWS);\n'
            '  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.sd_multi_args)
    for f in fields:
        assert getattr(_lib.sd_multi_args, f).offset == int(got[f]), f
    assert got["limits"].split() == [str(_lib.SD_MULTI_MAX_DRAFTS), str(_lib.SD_MULTI_MAX_NODES),
                                     str(_lib.SD_MULTI_MAX_ROWS)]
    assert _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12      # additive: the ABI number stays
