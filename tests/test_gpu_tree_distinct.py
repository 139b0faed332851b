"""GPU tests of the token-tree verify for distinct children (sd_verify_tree_distinct;
csrc/sd_verify_tree_distinct.inc): walks against the host model (tests/tree_distinct_ref.py over the
exact-arithmetic oracle and the numpy Philox) on cases built by tests/tree_distinct_walk.py, the edges
of the exclusions, row layouts, one-child trees against sd_verify_tree, losslessness over 4096
sequences, the greedy loop end to end, graph capture, workspace reuse and the torch op.

At most one row per case may differ from the host model, and only a row the host flagged close (an
accept test within 1e-6 of its threshold); the Philox offset of a case is chosen on the host so."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fakelm
import multi_walk as mw
import row_edges as rowe
import tree_distinct_ref as dref
import tree_distinct_walk as dw
import tree_walk as tw
from oracle import specdec_ref as ref
from test_gpu_perfmode import chi2_check
from test_gpu_tree import check_draw
from tree_ref import children_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7
FIELDS = ("n_accepted", "last_node", "next_token", "resample_mass", "n_sibling_rejects", "stop_index", "row_status",
          "path", "tokens_out")


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, TokenTree=TokenTree)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def run(sd, tl, tok, parent, proc, seed, off, row_base=0, stops=(), status_or=None):
    stop_t = torch.tensor(list(stops), dtype=torch.long, device=DEV)
    out = sd.ops.verify_tree_distinct(tl, tok, sd.TokenTree(parent), spec_of(sd, proc), sd.PhiloxNoise(seed=seed, offset=off),
                                      stop_tokens=stop_t, status_or=status_or, pad_token_id=PAD, row_base=row_base)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_TREE_DISTINCT == 9
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})


def check_case(sd, c, got, rows):
    L = sd.lib
    depth = max(tw.node_depths(c.parent))
    close_rows = 0
    for b, r in enumerate(rows):
        n, st, x = int(got.n_accepted[b]), int(got.row_status[b]), int(got.next_token[b])
        ints = (n, int(got.last_node[b]), int(got.n_sibling_rejects[b]), int(got.stop_index[b]), got.path[b].tolist())
        want = (r.n, r.last_node, r.rejects, r.stop_index, r.path + [-1] * (depth - r.n))
        print(f"[treed] b={b} got={ints} want={want} close={r.close} status=0x{st:x} x={x} host_x={r.x} "
              f"mass={float(got.resample_mass[b]):.6g}/{r.mass:.6g}")
        assert st & L.SD_ROW_DONE
        if ints != want:
            assert r.close, (b, ints, want)
            close_rows += 1
            continue
        row = got.tokens_out[b].tolist()
        assert row[:n] == [int(c.tok[b, i]) for i in r.path]
        want_bit = {dref.RESIDUAL: L.SD_ROW_RESIDUAL, dref.BONUS: L.SD_ROW_BONUS, dref.STOP: L.SD_ROW_STOP_IN_DRAFTS}
        assert st & (L.SD_ROW_RESIDUAL | L.SD_ROW_BONUS | L.SD_ROW_STOP_IN_DRAFTS) == want_bit[r.status], (b, hex(st))
        if r.mass == r.mass:
            tol = dw.mass_tolerance(c, b, r.slot)
            print(f"[treed-mass] b={b} excluded={len(r.excluded)} dev={abs(float(got.resample_mass[b]) - r.mass):.3g} bound={tol:.3g}")
            assert abs(float(got.resample_mass[b]) - r.mass) <= tol, (b, float(got.resample_mass[b]), r.mass, tol)
        else:
            assert np.isnan(float(got.resample_mass[b]))
        if r.status == dref.STOP:
            assert x == -1 and row[n:] == [PAD] * (depth + 1 - n) and not st & L.SD_ROW_ERROR_MASK
            continue
        if c.proc.stochastic and not (r.valid and r.final_mass > 0):
            assert st & L.SD_ROW_INVALID_DIST and x == -1 and row[n:] == [PAD] * (depth + 1 - n)
            continue
        assert not st & L.SD_ROW_ERROR_MASK
        assert 0 <= x < c.V and row[n] == x and row[n + 1:] == [PAD] * (depth - n)
        if c.proc.stochastic:
            assert r.weights[x] > 0, (b, x)          # never an excluded token, never one without weight
            check_draw(f"b={b}", r, x, dw.mass_tolerance(c, b, r.slot))
        else:
            assert x == r.x, (b, x, r.x)             # the argmax of the processed logits, lowest index first
    assert close_rows <= 1


# ---------------------------------------------------------------- walks against the host model
def _id(case):
    tname, V, dt, name = case
    return f"{tname}-V{V}-{str(dt).split('.')[-1]}-{name}"


@pytest.mark.parametrize("case", dw.grid(), ids=_id)
def test_walks_equal_the_host_model(sd, case):
    c = dw.case(*case)
    off, rows = dw.quiet_offset(c)
    cov = dw.coverage(rows)
    print(f"[treed] {_id(case)} offset={off} coverage={vars(cov)}")
    got = run(sd, c.tl.to(DEV), c.tok.to(DEV), c.parent, c.proc, dw.SEED, off, dw.ROW_BASE)
    check_case(sd, c, got, rows)


def test_stop_on_the_accepted_path(sd):
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    _, free = dw.quiet_offset(c)
    b_hit = next(b for b, r in enumerate(free) if r.n >= 2)
    stop, first = int(c.tok[b_hit, free[b_hit].path[1]]), int(c.tok[b_hit, free[b_hit].path[0]])
    stops = [c.V + 11, stop, first]                                   # listed later: the earlier-listed stop wins
    off, rows = dw.quiet_offset(c, stops)
    assert rows[b_hit].status == dref.STOP and rows[b_hit].stop_index == 1
    got = run(sd, c.tl.to(DEV), c.tok.to(DEV), c.parent, c.proc, dw.SEED, off, dw.ROW_BASE, stops)
    check_case(sd, c, got, rows)
    assert int(got.next_token[b_hit]) == -1


# ---------------------------------------------------------------- exclusion edges
def _edge_case(tl, tok, parent, proc_name):
    return dw.finish(tl, tok, parent, proc_name)


@pytest.mark.parametrize("dtype,name", [(torch.bfloat16, "multinomial"), (torch.float32, "multinomial_T0.7"),
                                        (torch.float16, "greedy")])
def test_children_at_the_chunk_edges(sd, dtype, name):
    """Children at ids 0, 2047, 2048 and V - 1 (V = 4101: three chunks), lifted so that they carry
    weight; sequences alternate between light and heavy children (accepting early, or rejecting all four)."""
    V, parent = 4101, tw.from_branching([4])
    g = torch.Generator().manual_seed(91)
    base = torch.randn(dw.B, 5, V, generator=g) * 3
    ids = [0, 2047, 2048, V - 1]
    base[:, 0, ids] = 10.5                                 # about a tenth of the row's mass each
    base[::2, 0, ids] = 8.5
    base[1::4, 0, ids[2]] = 14.0                           # the row maximum at the third child (greedy accepts it)
    tok = torch.tensor([ids] * dw.B)
    c = _edge_case(base.to(dtype), tok, parent, name)
    off, rows = dw.quiet_offset(c)
    cov = dw.coverage(rows)
    assert not c.proc.stochastic or (cov.resid_root >= 1 and cov.bonus >= 1), vars(cov)
    check_case(sd, c, run(sd, c.tl.to(DEV), c.tok.to(DEV), parent, c.proc, dw.SEED, off, dw.ROW_BASE), rows)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_chunk_that_holds_only_the_children(sd, dtype):
    """All children of the root lie in chunk 1, whose other entries are -inf: once they are rejected the
    chunk's remainder is exactly zero (or a rounding residue, which the draw must walk past): the token
    comes from another chunk, never an excluded one, and the row is not flagged."""
    V, parent = 4101, tw.from_branching([3])
    g = torch.Generator().manual_seed(17)
    base = torch.randn(dw.B, 4, V, generator=g) * 3
    ids = [2048 + 5, 2048 + 1000, 4095]
    base[:, 0, 2048:4096] = -math.inf
    base[:, 0, ids] = torch.randn(dw.B, 3, generator=g) - 1.0         # light children: mostly rejected
    base[:, 0, 4096:] += 8                                            # the short last chunk carries real mass
    tok = torch.tensor([ids] * dw.B)
    c = _edge_case(base.to(dtype), tok, parent, "multinomial")
    # the cdf uniform decides the chunk: take an offset at which some all-rejected row draws beyond chunk 1
    for start in range(dw.OFFSET, dw.OFFSET + 64):
        off, rows = dw.quiet_offset(c, start=start)
        if sum(r.status == dref.RESIDUAL and len(r.excluded) == 3 and r.x >= 4096 for r in rows) >= 1 \
                and sum(r.status == dref.RESIDUAL and len(r.excluded) == 3 and r.x < 2048 for r in rows) >= 1:
            break
    else:
        raise AssertionError("no offset reaches both sides of the emptied chunk")
    got = run(sd, c.tl.to(DEV), c.tok.to(DEV), parent, c.proc, dw.SEED, off, dw.ROW_BASE)
    check_case(sd, c, got, rows)
    for b, r in enumerate(rows):
        if r.status == dref.RESIDUAL:
            assert not 2048 <= int(got.next_token[b]) < 4096


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float16])
def test_the_whole_mass_on_the_children(sd, dtype):
    """The root's row is -inf but at its three children (in two chunks): whatever the uniforms, the last
    child with weight is accepted (its ratio is w / rem = 1) and no residual is ever drawn."""
    V, parent = 2049, tw.from_branching([3, 1])
    g = torch.Generator().manual_seed(23)
    base = torch.randn(dw.B, 7, V, generator=g) * 3
    ids = [7, 2047, 2048]
    base[:, 0] = -math.inf
    base[:, 0, ids] = torch.randn(dw.B, 3, generator=g)
    tok = torch.cat([torch.tensor([ids] * dw.B), torch.randint(0, V, (dw.B, 3), generator=g)], 1)
    c = _edge_case(base.to(dtype), tok, parent, "multinomial")
    off, rows = dw.quiet_offset(c)
    assert all(r.n >= 1 for r in rows) and any(r.path[0] == 2 for r in rows)
    got = run(sd, c.tl.to(DEV), c.tok.to(DEV), parent, c.proc, dw.SEED, off, dw.ROW_BASE)
    check_case(sd, c, got, rows)
    assert int((got.n_accepted >= 1).sum()) == dw.B


def test_duplicate_siblings_and_ids_outside_the_vocabulary(sd):
    """fan8 with children [a, a, -1, V, b, b, c, V + 5]: a repeat of a rejected sibling, and ids -1, V and
    V + 5, are rejected without weight (their uniforms unread, nothing excluded twice)."""
    V, parent = 1000, tw.from_branching([8])
    g = torch.Generator().manual_seed(29)
    base = torch.randn(dw.B, 9, V, generator=g) * 3
    abc = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(dw.B)])
    a, b_, c_ = abc[:, 0], abc[:, 1], abc[:, 2]
    tok = torch.stack([a, a, torch.full_like(a, -1), torch.full_like(a, V), b_, b_, c_, torch.full_like(a, V + 5)], 1)
    base[torch.arange(dw.B), 0, c_] = 11.0                             # the seventh child: about half the row's mass
    c = _edge_case(base.to(torch.bfloat16), tok, parent, "multinomial")
    off, rows = dw.quiet_offset(c)
    cov = dw.coverage(rows)
    assert cov.weightless >= dw.B // 2 and any(r.n == 1 and r.path == [6] for r in rows), vars(cov)
    check_case(sd, c, run(sd, c.tl.to(DEV), c.tok.to(DEV), parent, c.proc, dw.SEED, off, dw.ROW_BASE), rows)


def test_a_nan_target_row_is_flagged(sd):
    V, parent = 2049, tw.from_branching([2, 1])
    g = torch.Generator().manual_seed(31)
    tl = (torch.randn(4, 5, V, generator=g) * 3).to(torch.bfloat16)
    tl[1, 0, 2048] = math.nan                                          # the root's row of sequence 1
    tok = torch.randint(0, V, (4, 4), generator=g)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = run(sd, tl.to(DEV), tok.to(DEV), parent, mw.PROCS["multinomial"], 5, 1, status_or=err)
    L = sd.lib
    assert int(got.row_status[1]) & L.SD_ROW_INVALID_DIST and int(got.next_token[1]) == -1 and int(got.n_accepted[1]) == 0
    assert got.tokens_out[1].tolist() == [PAD] * 3
    assert int(err[0]) & L.SD_ROW_INVALID_DIST
    others = [0, 2, 3]
    assert all(not int(got.row_status[b]) & L.SD_ROW_ERROR_MASK and int(got.next_token[b]) >= 0 for b in others)


# ---------------------------------------------------------------- row layouts
@pytest.mark.parametrize("layout", rowe.LAYOUTS)
@pytest.mark.parametrize("tname,V,dtype,name", [("two-two", 2049, torch.bfloat16, "multinomial"), ("five", 1000, torch.float32, "topk50"),
                                                ("fan8", 4101, torch.float16, "greedy"), ("irregular64", 64, torch.bfloat16, "nucleus0.9")])
def test_rows_in_a_poisoned_buffer(sd, layout, tname, V, dtype, name):
    """Packed, padded and 2-byte-shifted (16-byte-misaligned) rows inside a buffer of NaN: an element
    outside a row that reaches a sum, a maximum or a draw shows as a wrong or flagged row."""
    c = dw.case(tname, V, dtype, name)
    off, rows = dw.quiet_offset(c)
    tl = rowe.place(c.tl, layout, math.nan, DEV)
    check_case(sd, c, run(sd, tl, c.tok.to(DEV), c.parent, c.proc, dw.SEED, off, dw.ROW_BASE), rows)


# ---------------------------------------------------------------- one child per slot: sd_verify_tree
@pytest.mark.parametrize("parent", [tw.chains(1, 8), [-1, 0, 1, 2]], ids=["chain8", "chain4"])
def test_one_child_trees_equal_sd_verify_tree_on_one_hot_drafts(sd, parent):
    """Every slot has at most one child: sd_verify_tree fed one-hot drafter rows (-inf everywhere but the
    child's id, so q(x) = 1) tests u > p(x), this rule u > p(x) / Z.  fp32, V = 1000, B = 64, the same
    seed and offset: n, path and status agree on every row the host model does not flag close, the
    slack widened by |Z - 1|."""
    B, V, N = 64, 1000, len(parent)
    g = torch.Generator().manual_seed(41)
    tl = torch.randn(B, N + 1, V, generator=g) * 2
    tok = torch.randint(0, V, (B, N), generator=g)
    tl[torch.arange(B)[:, None], torch.tensor(parent)[None] + 1, tok] += 7          # children the target likes: deep paths
    c = dw.finish(tl, tok, parent, "multinomial")
    tree = sd.TokenTree(parent)
    dl = torch.full((B, N + 1, V), -math.inf)
    dl[torch.arange(B)[:, None], torch.tensor(parent)[None] + 1, tok] = 0.0
    draft = [dl[:, s].to(DEV) if tree.children[s] else None for s in range(N + 1)]
    seed, off = 1234, 3
    a = run(sd, tl.to(DEV), tok.to(DEV), parent, c.proc, seed, off)
    o = sd.ops.verify_tree(tl.to(DEV), draft, tok.to(DEV), tree, spec_of(sd, c.proc), sd.PhiloxNoise(seed=seed, offset=off))
    rows = dw.host_results(c, seed=seed, off=off, row_base=0)
    compared = 0
    for b, r in enumerate(rows):
        slack = dref.CLOSE + max(abs(float(c.P[b, s].sum()) - 1) for s in range(N + 1))
        near = any(abs(float(dref.ph.accept_uniform(seed, off, b, cn)) - ratio) <= slack * max(1.0, ratio)
                   for cn, _, ratio, _ in r.tests)
        if near:
            continue
        compared += 1
        assert int(a.n_accepted[b]) == int(o.n_accepted[b]) == r.n, b
        assert a.path[b].tolist() == o.path[b].cpu().tolist(), b
        assert int(a.row_status[b]) == int(o.row_status[b]), b
    assert compared >= B - 2 and len({int(v) for v in a.n_accepted}) >= 3


# ---------------------------------------------------------------- losslessness on the device
def _rows(n_rows, V, seed, tail):
    g = torch.Generator().manual_seed(seed)
    tl = torch.randn(n_rows, V, generator=g) * 2
    noise = 0.8 * torch.randn(n_rows, V, generator=g)
    if tail:
        tl[:, mw.last_chunk_start(V):] += 8
    tl = tl.to(torch.bfloat16)
    dl = (tl.float() + noise).to(torch.bfloat16)
    return tl, dl, ref.process(tl, mw.PROCS["multinomial"], exact=True).double().numpy()


def _top(dl_rows, k):
    """[R, k] the top-k ids of every row, value descending, lowest index first."""
    return torch.from_numpy(np.stack([dref.topk_tokens(r.double().numpy(), k) for r in dl_rows]))


@pytest.mark.parametrize("V", [64, 1000, 4101])
def test_first_token_keeps_the_target_distribution(sd, V):
    """from_branching([4]): 4096 sequences with identical rows, the children the top-4 of a correlated
    drafter row; the first emitted token against the exact processed p."""
    B, parent = 4096, tw.from_branching([4])
    tl, dl, p = _rows(2, V, 5, V > tw.CHUNK)
    tok = _top(dl[:1], 4).expand(B, 4).contiguous()
    T = torch.stack([tl[0]] + [tl[1]] * 4).to(DEV).expand(B, 5, V).contiguous()
    out = sd.ops.verify_tree_distinct(T, tok.to(DEV), parent, spec_of(sd, mw.PROCS["multinomial"]),
                                      sd.PhiloxNoise(seed=99, offset=3), pad_token_id=PAD)
    first = out.tokens_out[:, 0].cpu().numpy()
    assert first.min() >= 0
    st = out.row_status.cpu().numpy()
    assert (st & sd.lib.SD_ROW_RESIDUAL != 0).sum() > 0 and (st & sd.lib.SD_ROW_BONUS != 0).sum() > B // 32
    chi2_check(first, p[0], f"treed [4] first token V={V}")


@pytest.mark.parametrize("V", [64, 1000, 4101])
def test_two_tokens_keep_the_target_distribution(sd, V):
    """from_branching([2, 2]) with context-dependent rows: the node that holds token a gets the rows of
    context a, its children the top-2 of the drafter's row of context a.  The first emitted token
    against the exact p of the root; the second, over the sequences whose first token is the most
    frequent accepted one a, against p(. | a).  (All sequences share the rows, so the tree is the same
    in all of them and the statistics are over the verify's noise alone, as the rule's argument is.)"""
    B, parent = 4096, tw.from_branching([2, 2])
    tl, dl, p = _rows(1 + V, V, 7, V > tw.CHUNK)          # row 0: the root; row 1 + a: context a
    t0 = _top(dl[:1], 2)[0]                               # the root's children
    t1 = _top(dl[1 + t0], 2)                              # [2, 2]: the children of the two depth-1 nodes
    tok1 = torch.cat([t0, t1.reshape(-1)])
    leaf_ctx = 1 + (t0.repeat_interleave(2) + t1.reshape(-1)) % V
    T1 = torch.cat([tl[:1], tl[1 + t0], tl[leaf_ctx]])
    T = T1.to(DEV).expand(B, 7, V).contiguous()
    out = sd.ops.verify_tree_distinct(T, tok1.to(DEV).expand(B, 6).contiguous(), parent, spec_of(sd, mw.PROCS["multinomial"]),
                                      sd.PhiloxNoise(seed=77, offset=9), pad_token_id=PAD)
    toks = out.tokens_out.cpu().numpy()
    first = toks[:, 0]
    assert first.min() >= 0
    chi2_check(first, p[0], f"treed [2,2] first token V={V}")
    n = out.n_accepted.cpu().numpy()
    a = int(np.bincount(first[n >= 1]).argmax())
    sel = (n >= 1) & (first == a)
    assert sel.sum() >= 50, sel.sum()
    chi2_check(toks[sel, 1], p[1 + a], f"treed [2,2] second token given {a} V={V}")


# ---------------------------------------------------------------- the greedy loop end to end
LOOP_V, LOOP_TOKENS = 4096, 40
PROMPT = [5, 17, 101, 9, 2000, 77]
BRANCHING = [3, 2, 1]


@pytest.fixture(scope="module")
def pair():
    from test_gpu_tree_loop import TreeFakeLM
    from specdec_amd.tree import TokenTree
    tree = TokenTree.from_branching(BRANCHING)
    t, d = fakelm.make_banks(LOOP_V, sigma=1.0, dtype=torch.float32)
    top2 = torch.topk(t, 2, dim=-1).values
    assert bool((top2[:, 0] > top2[:, 1]).all())          # every row maximum of the target is unique
    return TreeFakeLM(t.to(DEV), tree), TreeFakeLM(d.to(DEV), tree), tree


def _loop(pair, seed=3, **kw):
    from specdec_amd.sampling import tree_speculative_generate
    target, drafter, tree = pair
    torch.manual_seed(seed)
    return tree_speculative_generate(PROMPT, drafter, target, max_gen_len=LOOP_TOKENS, eos_tokens_id=[LOOP_V + 5], tree=tree, **kw)


def test_greedy_topk_loop_emits_the_targets_greedy_decode(pair):
    from specdec_amd.sampling.base_decoding import autoregressive_generate
    target = pair[0]
    want = autoregressive_generate(PROMPT, target, max_gen_len=LOOP_TOKENS, eos_tokens_id=[LOOP_V + 5])
    trace = []
    toks, rate = _loop(pair, children="topk", trace=trace)
    assert toks == want and len(toks) == LOOP_TOKENS
    sampled, rate_s = _loop(pair)                          # greedy iid children: every sibling is the drafter's argmax
    s_trace = []
    _loop(pair, trace=s_trace)
    assert all(len({int(t) for t in st["draft_tokens"][:3]}) == 1 for st in s_trace)
    print(f"[treed-loop] greedy accepted/speculated: topk {rate:.3f}, sample {rate_s:.3f}")
    assert rate > rate_s
    assert any(st["path"] and st["path"][0] != 0 for st in trace)      # a second-best child was accepted somewhere
    # children are distinct at every slot
    ch = children_of(trace[0]["parent"])
    assert all(len({int(st["draft_tokens"][c]) for c in cs}) == len(cs) for st in trace for cs in children_of(st["parent"]) if cs)
    assert ch[0] == [0, 1, 2]


def test_sample_children_are_unchanged_by_the_new_keyword(pair):
    """children omitted and children="sample": the same trace, bit for bit, under a stochastic processor."""
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    a, b = [], []
    ta = _loop(pair, seed=21, logits_processor=MultinomialProcessor(1.0), trace=a)
    tb = _loop(pair, seed=21, logits_processor=MultinomialProcessor(1.0), trace=b, children="sample")
    assert ta == tb and len(a) == len(b)
    for x, y in zip(a, b):
        assert {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in x.items()} == \
               {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in y.items()}


def test_cached_topk_loops_emit_the_uncached_tokens():
    """Tiny fp32 Llamas (the cached tree loop's): children="topk" under greedy gives the target's
    greedy decode with no cache, a DynamicCache and a StaticCache alike."""
    from test_gpu_tree_cached_loop import GEN, PROMPT as P2, _tiny_llama
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.sampling.base_decoding import autoregressive_generate
    from specdec_amd.tree import TokenTree
    target = _tiny_llama(1).to(DEV)
    drafter = _tiny_llama(2, noise_of=target).to(DEV)
    tree = TokenTree.from_branching(BRANCHING)
    want = autoregressive_generate(P2, target, max_gen_len=GEN, eos_tokens_id=[-1])
    runs = {}
    for kind, kw in {"uncached": {}, "dynamic": dict(use_cache=True), "static": dict(use_cache=True, static_cache=True)}.items():
        torch.manual_seed(11)
        runs[kind] = tree_speculative_generate(P2, drafter, target, max_gen_len=GEN, eos_tokens_id=[-1], tree=tree,
                                               children="topk", **kw)
        print(f"[treed-loop] llama {kind}: rate {runs[kind][1]:.3f}")
    assert runs["uncached"][0] == runs["dynamic"][0] == runs["static"][0]
    assert runs["uncached"][1] == runs["dynamic"][1] == runs["static"][1] > 0
    with torch.no_grad():                                              # greedy = the target's decode where its maxima are unique
        seq = torch.tensor([P2 + runs["uncached"][0]], device=DEV)
        top2 = torch.topk(target(input_ids=seq).logits[0].float(), 2, dim=-1).values
    assert bool((top2[:, 0] > top2[:, 1]).all())
    assert runs["uncached"][0] == want


# ---------------------------------------------------------------- call-level checks
def test_capture_and_replay_with_an_advanced_offset(sd):
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    tree = sd.TokenTree(c.parent)
    tl, tok = c.tl.to(DEV), c.tok.to(DEV)
    spec = spec_of(sd, c.proc)
    replay_off, rows = dw.quiet_offset(c, start=dw.OFFSET + 6)
    off = torch.tensor([0], dtype=torch.long, device=DEV)
    noise = sd.PhiloxNoise(seed=dw.SEED, offset=0, offset_dev=off)   # the eager call takes host offset 0, the captured one 1
    eager = sd.ops.verify_tree_distinct(tl, tok, tree, spec, noise, pad_token_id=PAD, row_base=dw.ROW_BASE)   # sizes the workspace
    want0 = {f: getattr(eager, f).clone() for f in FIELDS}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sd.ops.verify_tree_distinct(tl, tok, tree, spec, noise, pad_token_id=PAD, row_base=dw.ROW_BASE)
    off.fill_(replay_off - 1)
    graph.replay()
    torch.cuda.synchronize()
    got = SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})
    check_case(sd, c, got, rows)
    assert not all(torch.equal(torch.nan_to_num(getattr(got, f).float(), nan=-1.0),
                               torch.nan_to_num(want0[f].cpu().float(), nan=-1.0)) for f in FIELDS)


def test_one_workspace_serves_mixed_entry_points(sd):
    shapes = [("irregular64", 2049, torch.bfloat16, "multinomial"), ("five", 64, torch.float32, "topk50"),
              ("fan8", 4101, torch.float16, "greedy")]
    cases = [dw.case(*s) for s in shapes]
    go = lambda c: run(sd, c.tl.to(DEV), c.tok.to(DEV), c.parent, c.proc, dw.SEED, dw.OFFSET, dw.ROW_BASE)  # noqa: E731
    first = [go(c) for c in cases]
    spec = sd.ops.ProcSpec("multinomial", 1.0)
    t = tw.case(33, "b4211", 2049, torch.bfloat16, "multinomial", True)
    ttree = sd.TokenTree(t.parent)
    for rnd in range(2):
        for c, want in zip(cases, first):
            x = c.tl.to(DEV)
            sd.ops.verify([x[:, 0], x[:, 1]], [x[:, 1]], c.tok[:, :1].clamp(0, c.V - 1).contiguous().to(DEV), sd.lib.SD_RULE_SPEC,
                          spec, spec, sd.PhiloxNoise(seed=1, offset=rnd))
            sd.ops.sample_rows(x[:, 0].contiguous(), spec, sd.PhiloxNoise(seed=2, offset=rnd))
            sd.ops.verify_tree(t.tl.to(DEV), t.dl[:, ttree.internal_slots].contiguous().to(DEV), t.tok.to(DEV), ttree,
                               spec_of(sd, t.proc), sd.PhiloxNoise(seed=3, offset=rnd))
            again = go(c)
            for f in FIELDS:
                a, w = getattr(again, f), getattr(want, f)
                if f == "resample_mass":
                    a, w = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(w, nan=-1.0)
                assert torch.equal(a, w), f


def test_torch_op_equals_ops_verify_tree_distinct(sd):
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    tl, tok = c.tl.to(DEV), c.tok.to(DEV)
    stops = torch.tensor([int(c.tok[2, 0])], dtype=torch.long, device=DEV)
    want = sd.ops.verify_tree_distinct(tl, tok, c.parent, spec_of(sd, c.proc), sd.PhiloxNoise(seed=dw.SEED, offset=dw.OFFSET),
                                       stop_tokens=stops, row_base=dw.ROW_BASE)
    got = torch.ops.specdec.verify_tree_distinct(tl, tok, c.parent, stops, sd.ops.KIND[c.proc.kind], c.proc.temperature,
                                                 c.proc.top_k, c.proc.top_p, dw.SEED, dw.OFFSET, dw.ROW_BASE)
    for g, f in zip(got, sd.ops.TREE_FIELDS + ("path",)):
        w = getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, f
        assert torch.equal(torch.nan_to_num(g.float(), nan=-1.0), torch.nan_to_num(w.float(), nan=-1.0)), f


def test_topk_children_and_a_user_processor(sd):
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 4101, generator=g) * 3
    x[0, [7, 900, 4100]] = 40.0                                        # equal values: index ascending
    got = sd.ops.topk_children(x.to(DEV), 4).cpu()
    assert got.shape == (5, 4) and got.dtype == torch.long
    assert got[0, :3].tolist() == [7, 900, 4100]
    for r in range(1, 5):
        assert got[r].tolist() == dref.topk_tokens(x[r].double().numpy(), 4)

    class Mine(MultinomialProcessor):
        def _process(self, logits):
            return logits

    with pytest.raises(TypeError):
        sd.ops.verify_tree_distinct(x[None, :2].to(DEV), torch.zeros(1, 1, dtype=torch.long, device=DEV), [-1], Mine(1.0),
                                    sd.PhiloxNoise(seed=1, offset=0))
