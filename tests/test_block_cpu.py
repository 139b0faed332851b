"""CPU checks of the block verify: the rule itself (exact enumeration on the host model against the
target's joint distribution, the expected accepted count against the token-wise rule's), γ' = 1 against
the multi-draft host model at one chain, the w == 0 and 0/0 conventions, the coverage of the GPU cases
(tests/test_gpu_block.py runs block_cases.grid()), the margin of the statistical GPU test, the C ABI's
layout and argument checks through ctypes, and the torch op's fake implementation."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import block_cases as bc
import block_ref as br
import multidraft_ref as mref


# ---------------------------------------------------------------- the rule is lossless
def _ctx_rows(V, seed, zeros=False):
    """Context-dependent p and q: a distribution per prefix; with `zeros`, one entry of each at 0."""
    def dist(prefix, which):
        r = np.random.default_rng([seed, which, len(prefix)] + list(prefix))
        v = r.random(V) + 0.05
        if zeros:
            v[r.integers(V)] = 0.0
        return v / v.sum()

    return (lambda pre: dist(pre, 0)), (lambda pre: dist(pre, 1))


def _enumerate(V, g, seed, zeros):
    """(largest deviation of the joint of the first γ+1 emitted tokens from the target's, block E[n],
    token-wise E[n]) over every draft (weighted by its probability under q) and every outcome of
    block_ref.walk; a step that emitted fewer than γ+1 tokens is continued by the target's rows."""
    p_of, q_of = _ctx_rows(V, seed, zeros)
    joint, eb, et = {}, 0.0, 0.0

    def extend(prefix, prob):
        if len(prefix) == g + 1:
            joint[tuple(prefix)] = joint.get(tuple(prefix), 0.0) + prob
            return
        pp = p_of(list(prefix))
        for x in range(V):
            if pp[x] > 0:
                extend(prefix + [x], prob * pp[x])

    for tok in itertools.product(range(V), repeat=g):
        pr = float(np.prod([q_of(list(tok[:d]))[tok[d]] for d in range(g)]))
        if pr == 0:
            continue
        P = np.array([p_of(list(tok[:d])) for d in range(g + 1)])
        Q = np.array([q_of(list(tok[:d])) for d in range(g)])
        for po, o in br.enumerate_outcomes(P, Q, tok):
            eb += pr * po * o.n
            assert o.final_mass > 0
            w = o.weights / o.final_mass
            for x in range(V):
                if w[x] > 0:
                    extend(list(tok[:o.n]) + [x], pr * po * w[x])
        et += pr * br.tokenwise_expectation(P, Q, tok)
    err = 0.0
    for seq in itertools.product(range(V), repeat=g + 1):
        want = float(np.prod([p_of(list(seq[:d]))[seq[d]] for d in range(g + 1)]))
        err = max(err, abs(joint.get(seq, 0.0) - want))
    return err, eb, et


TABLES = [(V, g, zeros) for V in (2, 3, 4) for g in (1, 2, 3, 4) for zeros in (False, True) if V ** g <= 256]


@pytest.mark.parametrize("V,g,zeros", TABLES)
def test_exact_enumeration_reproduces_the_target_joint(V, g, zeros):
    """The emitted tokens, continued by the target, reproduce the target's joint distribution to 1e-12;
    the expected accepted count is at least the token-wise rule's; at γ' = 1 the two coincide."""
    err, eb, et = _enumerate(V, g, 7 + V + g, zeros)
    print(f"V={V} g={g} zeros={zeros}: joint deviation {err:.3g}, E[n] block {eb:.4f} token-wise {et:.4f}")
    assert err < 1e-12
    assert eb >= et - 1e-12
    if g == 1:
        assert abs(eb - et) < 1e-12


# ---------------------------------------------------------------- γ' = 1 is the single-chain walk
def test_one_draft_equals_the_multidraft_host_model_at_one_chain():
    c = bc.case(16, 1, 2049, torch.bfloat16, "multinomial")
    for b in range(c.B):
        P, Q, tok = c.P[b].double().numpy(), c.Q[b].double().numpy(), c.tok[b].numpy()
        r = c.rows[b]
        m = mref.philox_step(P[None], Q[None], tok[None], bc.SEED, bc.OFFSET, bc.ROW_BASE + b, c.stops)
        assert (r.n, r.status, r.stop_index, r.prune_drafter, r.prune_target) == \
            (m.n, m.status, m.stop_index, m.prune_drafter, m.prune_target)
        assert r.x == m.x and r.emitted == m.emitted
        assert (math.isnan(r.mass) and math.isnan(m.mass)) or r.mass == m.mass
        assert np.array_equal(r.weights, m.weights)


# ---------------------------------------------------------------- conventions
def test_zero_weight_and_zero_over_zero_conventions():
    p = np.array([[0.5, 0.5, 0.0], [0.2, 0.3, 0.5], [0.1, 0.1, 0.8], [1 / 3, 1 / 3, 1 / 3]])
    q = np.array([[0.25, 0.25, 0.5], [0.0, 0.5, 0.5], [0.3, 0.3, 0.4]])
    # a zero ratio makes the weight 0 and it stays 0, even through an infinite ratio (0 * inf is no NaN)
    w = br.weights(p, q, [2, 0, 2])
    assert w == [1.0, 0.0, 0.0, 0.0]
    # 0/0 counts as +inf: the weight recovers to 1, as SPEC's test accepts there
    pz, qz = p.copy(), q.copy()
    pz[1, 0] = 0.0
    assert br.ratio(0.0, 0.0) == math.inf and br.ratio(0.3, 0.0) == math.inf and br.ratio(0.0, 0.3) == 0.0
    assert br.weights(pz, qz, [0, 0, 0])[:3] == [1.0, 1.0, 1.0]
    # an id outside the vocabulary has p = q = 0
    assert br.weights(p, q, [-1, 3, 7]) == [1.0, 1.0, 1.0, 1.0]
    assert br.tokenwise_n(p, q, [-1, 3, 7], [0.99, 0.99, 0.99]) == 3
    # no weight is ever NaN, h of a vanishing divisor is 0, and w = 0 leaves S = 0, h = 0
    w, S, h = br.rule(p, q, [2, 0, 2])
    assert not any(math.isnan(v) for v in w) and S[1] == 0.0 and S[2] == 0.0 and h[1] == 0.0 and h[3] == 0.0
    assert br.accept_prob(0.0, 1.0) == 0.0 and br.accept_prob(0.25, 1.0) == 1.0
    # with every test failed the walk exits at 0 on max(P_0 - Q_0, 0)
    o = br.walk(p, q, [2, 0, 2], lambda t, hh: False)
    assert o.n == 0 and o.status == br.RESIDUAL and np.allclose(o.weights, [0.25, 0.25, 0.0])


# ---------------------------------------------------------------- coverage of the GPU grid
def test_gpu_grid_reaches_every_scenario():
    """Every γ' >= 2 of the grid reaches each scenario in some case of that γ': a reject at 0, a reject
    at depth, a full accept, a stop among the accepted drafts, iid drafts and a rescue (n above the
    token-wise walk's on the same uniforms).  At least 20 rescue sequences overall; at most 5 % of the
    grid's sequences are close, and no case is all close."""
    groups, total, close, rescue = {}, 0, 0, 0
    grid = bc.grid()
    assert {c[2] for c in grid} >= {37, 2047, 2048, 2049, 4100, 128256}
    assert {c[1] for c in grid} == {1, 2, 4, 32} and {c[0] for c in grid} >= {1, 5, 16}
    assert bc.SERVING in grid
    for g in (1, 2, 4, 32):
        assert {c[3] for c in grid if c[1] == g} == set(bc.DTYPES)
    assert {c[4] for c in grid} == set(bc.PROCS)
    assert all(c[3] != torch.float16 or not ("topk" in c[4] or "nucleus" in c[4]) for c in grid)
    assert sum(c[5] != "none" for c in grid) >= len(grid) // 4 and {c[6] for c in grid} == {"packed", "padded", "shifted"}
    for key in grid:
        c = bc.case(*key)
        cov = bc.coverage(c)
        total += c.B
        close += cov.close
        rescue += cov.rescue
        assert cov.close < c.B, key
        acc = groups.setdefault(c.gamma, {k: 0 for k in vars(cov)})
        for k, v in vars(cov).items():
            acc[k] += v
        assert all(r.rescue == (r.n > r.tokenwise_n) for r in c.rows)
    for g, acc in groups.items():
        print(f"γ'={g}: {acc}")
        if g >= 2:
            assert all(acc[k] >= 1 for k in ("rej0", "rej_deep", "full", "stop", "iid", "rescue")), (g, acc)
    print(f"{total} sequences, {close} close, {rescue} rescues")
    assert rescue >= 20
    assert close <= 0.05 * total


def test_h_bounds_hold_the_host_values_and_tighten_with_the_tolerances():
    """accept_bounds brackets the host's own h, is exact where nothing can move (t = γ' at w = 1 stays
    within the weight bound) and widens with the mass tolerance."""
    c = bc.case(16, 4, 2048, torch.float16, "multinomial")
    for b, r in enumerate(c.rows):
        for t in range(1, c.gamma + 1):
            assert r.h_lo[t] <= r.h[t] <= r.h_hi[t]
            assert r.h_hi[t] - r.h_lo[t] >= 0
        for t in range(1, c.gamma):
            lo1, hi1 = br.accept_bounds(r.S[t], r.w[t], t, c.gamma, c.s_tol[b][t])
            lo2, hi2 = br.accept_bounds(r.S[t], r.w[t], t, c.gamma, 10 * c.s_tol[b][t])
            assert lo2 <= lo1 + 1e-12 and hi2 >= hi1 - 1e-12
    assert br.weight_bound(0) == 0 and br.weight_bound(32) < 1e-4


# ---------------------------------------------------------------- the statistical GPU test's margin
def test_statistical_pair_separates_the_two_rules():
    """On block_cases.stat_pair (V = 8, γ' = 4, B = 16384) the block rule's exact expected accepted count
    exceeds the token-wise rule's by more than 8 standard errors of the GPU test's mean: that test's
    4-standard-error window cannot hold a token-wise walk."""
    eb, et, se = bc.stat_expectations()
    print(f"E[n] block {eb:.4f}, token-wise {et:.4f}, standard error {se:.5f}: {(eb - et) / se:.1f} se apart")
    assert eb - et > 8 * se


# ---------------------------------------------------------------- C ABI (ctypes)
def test_verify_block_rejects_bad_arguments_before_any_hip_call():
    from specdec_amd import _lib
    lib = _lib.lib
    for name in ("sd_verify_block_workspace_size", "sd_verify_block"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.sd_verify_block(None, None) == _lib.SD_ERR_INVALID
    a = _lib.sd_block_args()
    a.batch, a.gamma, a.vocab = 1, 4, 100
    a.proc = _lib.sd_processor(_lib.SD_PROC_MULTINOMIAL, 1.0, 0, 1.0)
    a.noise.mode = _lib.SD_NOISE_PHILOX
    assert lib.sd_verify_block(C.byref(a), None) == _lib.SD_ERR_INVALID      # null pointers
    assert lib.sd_verify_block_workspace_size(1, 4, 100) > 0
    for shape in ((0, 4, 100), (1, 0, 100), (1, 33, 100), (16385, 4, 100), (1, 4, 0)):
        assert lib.sd_verify_block_workspace_size(*shape) == 0, shape
    assert lib.sd_verify_block_workspace_size(16384, 4, 100) > 0
    assert _lib.SD_PATH_VERIFY_BLOCK == 11 and _lib.SD_PATH_VERIFY_BLOCK in _lib.PATH_NAMES


def test_block_args_ctypes_layout_matches_the_header():
    """sizeof and field offsets of sd_block_args: the ctypes mirror against the C header (gcc)."""
    import os
    import subprocess
    import tempfile
    from specdec_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.sd_block_args._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
            '  printf("size %zu\\n", sizeof(sd_block_args));\n'
            + "".join(f'  printf("{f} %zu\\n", offsetof(sd_block_args, {f}));\n' for f in fields)
            + '  printf("path %d\\n", (int)SD_PATH_VERIFY_BLOCK);\n'
            '  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.sd_block_args)
    for f in fields:
        assert getattr(_lib.sd_block_args, f).offset == int(got[f]), f
    assert int(got["path"]) == _lib.SD_PATH_VERIFY_BLOCK
    assert _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12      # additive: the ABI number stays


# ---------------------------------------------------------------- torch op, loop surface
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_verify_block_op_fake_shapes(dtype):
    import specdec_amd  # noqa: F401  (registers the ops)
    B, g, V = 3, 5, 128256
    t = torch.empty(B, g + 1, V, device="meta", dtype=dtype)
    d = torch.empty(B, g, V, device="meta", dtype=dtype)
    tok = torch.empty(B, g, device="meta", dtype=torch.long)
    stops = torch.empty(2, device="meta", dtype=torch.long)
    out = torch.ops.specdec.verify_block(t, d, tok, stops, 1, 1.0, 0, 1.0, 7, 0, 0)
    assert len(out) == 9
    want = [torch.int32, torch.long, torch.float32] + [torch.int32] * 4
    for o, dt in zip(out[:7], want):
        assert (o.shape, o.dtype, o.device.type) == ((B,), dt, "meta")
    assert (out[7].shape, out[7].dtype) == ((B, g + 1), torch.float32)
    assert (out[8].shape, out[8].dtype) == ((B, g), torch.float32)


def test_loop_is_exported_and_refuses_user_processors():
    from specdec_amd.sampling import block_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor

    class Own(MultinomialProcessor):
        def _process(self, logits):
            return logits

    class OwnSample(MultinomialProcessor):
        def sample(self, probs):
            return probs.argmax(-1)

    for proc in (Own(1.0), OwnSample(1.0)):
        with pytest.raises(TypeError):
            block_speculative_generate([1, 2], None, None, logits_processor=proc)
    with pytest.raises(ValueError):
        block_speculative_generate([1, 2], None, None, gamma=0)


def test_block_rule_gains_on_the_loop_tests_pair():
    """What the device loop's acceptance gain rests on: on the GPU loop test's FakeLM pair (vocab 4096,
    sigma 1, multinomial, γ = 4) the host model accepts more drafts per step under the block rule than
    under the token-wise one on the same stream of numpy noise."""
    import fakelm
    target, drafter = fakelm.make_pair(4096, sigma=1.0)
    blk = sum(bc.simulate_acceptance(target, drafter, 4, 200, s, block=True) for s in range(2)) / 2
    tokw = sum(bc.simulate_acceptance(target, drafter, 4, 200, s, block=False) for s in range(2)) / 2
    print(f"accepted drafts per step: block {blk:.3f}, token-wise {tokw:.3f}")
    assert blk > tokw
