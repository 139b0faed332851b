"""GPU tests of the token-tree verify (sd_verify_tree; csrc/sd_verify_tree.inc): walks against the
host model (tests/tree_ref.py over the exact-arithmetic oracle and the numpy Philox) with drafts
chosen by the test (tests/tree_walk.py; tests/test_tree_cpu.py proves what the cases reach), chains
against sd_verify and sd_verify_multi, stop lists, losslessness over 4096 sequences, workspace reuse,
graph capture and row layouts.

At most one row per case may differ from the host model, and only a row the host flagged close (an
accept test within the device's fp32 tolerance of its threshold)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import multi_walk as mw
import multidraft_ref as mref
import row_edges as rowe
import tree_ref as tref
import tree_walk as tw
from oracle import specdec_ref as ref
from test_gpu_perfmode import chi2_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, TokenTree=TokenTree)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


FIELDS = ("n_accepted", "last_node", "next_token", "resample_mass", "n_sibling_rejects", "stop_index", "row_status",
          "path", "tokens_out")


def run_tree(sd, tl, dl, tok, parent, proc, seed, off, row_base=0, stops=(), one_by_one=False):
    """verify_tree on device tensors tl [B, N+1, V], dl [B, N+1, V] (leaf slots' rows are not passed);
    one_by_one: one call per sequence (batch 1, global row row_base + b)."""
    tree = sd.TokenTree(parent)
    stop_t = torch.tensor(list(stops), dtype=torch.long, device=DEV)

    def call(sl, base):
        draft = [dl[sl, s] if tree.children[s] else None for s in range(tree.num_nodes + 1)]
        out = sd.ops.verify_tree(tl[sl], draft, tok[sl], tree, spec_of(sd, proc), sd.PhiloxNoise(seed=seed, offset=off),
                                 stop_tokens=stop_t, row_base=base, pad_token_id=PAD)
        assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_TREE
        return {f: getattr(out, f).cpu() for f in FIELDS}

    if one_by_one:
        outs = [call(slice(b, b + 1), row_base + b) for b in range(tl.shape[0])]
        return SimpleNamespace(**{f: torch.cat([o[f] for o in outs]) for f in FIELDS})
    return SimpleNamespace(**call(slice(None), row_base))


def check_draw(what, r, x, slack):
    """The device's token x against the host model's inverse CDF on the same uniform: the host's
    target u·Σ lies in the running-total interval of x, widened by 2·slack (multi_walk.draw_excess)."""
    lo, hi = mref.draw_interval(r.weights, x)
    used = mw.draw_excess(r, x, slack)
    print(f"[tree-draw] {what} {r.status} x={x} host_x={r.x} chunk={x // tw.CHUNK} target={r.u * r.total:.9g} "
          f"lo={lo:.9g} hi={hi:.9g} slack={slack:.3g} used={used:.3g}")
    assert used <= 1.0, (what, x, r.x, r.u * r.total, lo, hi, slack)


def check_case(sd, c, got, rows):
    L = sd.lib
    depth = max(tw.node_depths(c.parent))
    close_rows = 0
    for b, r in enumerate(rows):
        n, st, x = int(got.n_accepted[b]), int(got.row_status[b]), int(got.next_token[b])
        ints = (n, int(got.last_node[b]), int(got.n_sibling_rejects[b]), int(got.stop_index[b]), got.path[b].tolist())
        want = (r.n, r.last_node, r.rejects, r.stop_index, r.path + [-1] * (depth - r.n))
        print(f"[tree] b={b} got={ints} want={want} close={r.close} status=0x{st:x} x={x} "
              f"mass={float(got.resample_mass[b]):.6g}/{r.mass:.6g}")
        assert st & L.SD_ROW_DONE
        if ints != want:
            assert r.close, (b, ints, want)
            close_rows += 1
            continue
        row = got.tokens_out[b].tolist()
        assert row[:n] == [int(c.tok[b, i]) for i in r.path]
        if r.status != tref.STOP and c.proc.stochastic and not r.final_mass > 0:
            # zero mass left (small vocabularies): torch.multinomial raises, the row is flagged
            assert st & L.SD_ROW_INVALID_DIST and x == -1 and row[n:] == [PAD] * (depth + 1 - n)
            continue
        assert not st & L.SD_ROW_ERROR_MASK
        want_bit = {tref.RESIDUAL: L.SD_ROW_RESIDUAL, tref.BONUS: L.SD_ROW_BONUS, tref.STOP: L.SD_ROW_STOP_IN_DRAFTS}
        assert st & (L.SD_ROW_RESIDUAL | L.SD_ROW_BONUS | L.SD_ROW_STOP_IN_DRAFTS) == want_bit[r.status], (b, hex(st))
        if r.rejects:
            tol = tw.mass_tolerance(c, b, r)
            print(f"[tree-mass] b={b} rejects_at_slot={len(r.masses)} dev={abs(float(got.resample_mass[b]) - r.mass):.3g} "
                  f"bound={tol:.3g} mass={r.mass:.6g}")
            assert abs(float(got.resample_mass[b]) - r.mass) <= tol, (b, float(got.resample_mass[b]), r.mass, tol)
        else:
            assert np.isnan(float(got.resample_mass[b]))
        if r.status == tref.STOP:
            assert x == -1 and row[n:] == [PAD] * (depth + 1 - n)
            continue
        assert 0 <= x < c.V and row[n] == x and row[n + 1:] == [PAD] * (depth - n)
        if c.proc.stochastic:
            assert r.weights[x] > 0, (b, x)          # positive weight in the final residual / leaf row
            check_draw(f"b={b}", r, x, tw.draw_slack(c, b, r))
        else:
            assert r.weights[x] >= r.weights.max() * (1 - 1e-4), (b, x, r.x)
    assert close_rows <= 1


# ---------------------------------------------------------------- walks against the host model
def _id(case):
    B, tname, V, dt, name, tail = case[:6]
    return f"B{B}-{tname}-V{V}-{str(dt).split('.')[-1]}-{name}" + ("-tail" if tail else "")


@pytest.mark.parametrize("case", tw.grid(), ids=_id)
def test_walks_equal_the_host_model(sd, case):
    c = tw.case(*case)
    rows = tw.host_results(c)
    got = run_tree(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.parent, c.proc, tw.SEED, tw.OFFSET, tw.ROW_BASE,
                   one_by_one=case[0] == 1)
    check_case(sd, c, got, rows)


# ---------------------------------------------------------------- chains are sd_verify / sd_verify_multi
@pytest.mark.parametrize("name,V,dtype,g", [("multinomial", 4096, torch.bfloat16, 4), ("topk50", 1000, torch.float32, 4),
                                            ("greedy", 50257, torch.float16, 4), ("multinomial_T0.7", 2049, torch.bfloat16, 32)])
def test_one_chain_equals_sd_verify(sd, name, V, dtype, g):
    """chains(1, γ): every integer output of sd_verify(SD_RULE_SPEC) but next_token (whose draw uses
    one uniform here, two in sd_verify)."""
    c = mw.case(16, 1, g, V, dtype, name)
    stops = [int(c.tok[3, 0, 0])]
    tl, dl = c.tl[:, 0].to(DEV), c.dl[:, 0].to(DEV)
    got = run_tree(sd, tl, torch.cat([dl, dl[:, :1]], 1), c.tok[:, 0].to(DEV), tw.chains(1, g), c.proc, mw.SEED, mw.OFFSET,
                   mw.ROW_BASE, stops)
    spec = spec_of(sd, c.proc)
    one = sd.ops.verify([tl[:, t] for t in range(g + 1)], [dl[:, t] for t in range(g)], c.tok[:, 0].to(DEV),
                        sd.lib.SD_RULE_SPEC, spec, spec, sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET),
                        torch.tensor(stops, dtype=torch.long, device=DEV), row_base=mw.ROW_BASE)
    for f in ("n_accepted", "stop_index", "row_status"):
        assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f
    assert torch.equal(got.last_node, got.n_accepted - 1)
    assert torch.equal(got.n_sibling_rejects, (one.n_accepted.cpu() < g).int())   # one failed test ends a chain
    assert int((one.row_status.cpu() & sd.lib.SD_ROW_STOP_IN_DRAFTS != 0).sum()) >= 1


def _distinct_roots(c):
    """c.tok with pairwise distinct depth-0 tokens in every sequence (a repeated one becomes the likeliest
    unused token of the shared depth-0 drafter row): there the K-chains tree walks as the multi-draft
    prefix tree does (equal depth-0 tokens merge chains in sd_verify_multi only)."""
    tok = c.tok.clone()
    for b in range(c.B):
        best = torch.argsort(c.Q[b, 0, 0], descending=True).tolist()
        used = set()
        for k in range(c.K):
            t = int(tok[b, k, 0])
            if t in used:
                t = next(v for v in best if v not in used)
            used.add(t)
            tok[b, k, 0] = t
    return tok


def _chain_tree_inputs(c, bs):
    """Slot rows and node tokens of the K-chains tree (node d*K + k) from a multi_walk case."""
    K, g = c.K, c.gamma
    tl = torch.stack([c.tl[bs, 0, 0]] + [c.tl[bs, k, d + 1] for d in range(g) for k in range(K)], 1)
    dl = torch.stack([c.dl[bs, 0, 0]] + [c.dl[bs, k, min(d + 1, g - 1)] for d in range(g) for k in range(K)], 1)
    tok = torch.stack([c.tok[bs, k, d] for d in range(g) for k in range(K)], 1)
    return tl, dl, tok


def _same_root_rows(c):
    """A multi_walk case whose chains share the depth-0 rows, as the tree's root slot has one row pair."""
    tl, dl = c.tl.clone(), c.dl.clone()
    tl[:, :, 0] = tl[:, :1, 0]
    dl[:, :, 0] = dl[:, :1, 0]
    return tl, dl


@pytest.mark.parametrize("K,g,V,dtype,name", [(2, 4, 4096, torch.bfloat16, "multinomial"), (4, 4, 1000, torch.float32, "topk50"),
                                              (8, 2, 4097, torch.float16, "multinomial_T0.7"), (3, 5, 4096, torch.bfloat16, "greedy")])
def test_chains_equal_sd_verify_multi(sd, K, g, V, dtype, name):
    """chains(K, γ) on sequences with distinct depth-0 tokens: sd_verify_multi's n, winner (as
    last_node % K), rejects, status and stop_index exactly; the same next_token except in at most one
    row, which must then pass check_draw."""
    c0 = mw.case(16, K, g, V, dtype, name)
    tl_m, dl_m = _same_root_rows(c0)
    c = SimpleNamespace(**{**vars(c0), "tl": tl_m, "dl": dl_m})
    c.tok = _distinct_roots(c)
    bs = list(range(c.B))
    stops = [int(c.tok[1, 0, 0])]
    stop_t = torch.tensor(stops, dtype=torch.long, device=DEV)
    multi = sd.ops.verify_multi(tl_m[bs].to(DEV), dl_m[bs].to(DEV), c.tok[bs].to(DEV), spec_of(sd, c.proc),
                                sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET), stop_tokens=stop_t, row_base=3)
    tl, dl, tok = _chain_tree_inputs(c, bs)
    parent = tw.chains(K, g)
    got = run_tree(sd, tl.to(DEV), dl.to(DEV), tok.to(DEV), parent, c.proc, mw.SEED, mw.OFFSET, 3, stops)
    n = multi.n_accepted.cpu()
    assert torch.equal(got.n_accepted, n)
    win = multi.winner.cpu()
    has = n > 0
    assert torch.equal(got.last_node[has] % K, win[has]) and torch.equal(got.last_node[has] // K, n[has] - 1)
    assert torch.equal(got.n_sibling_rejects, multi.n_sibling_rejects.cpu())
    assert torch.equal(got.row_status, multi.row_status.cpu())
    assert torch.equal(got.stop_index, multi.stop_index.cpu())
    diff = (got.next_token != multi.next_token.cpu()).nonzero().flatten().tolist()
    assert len(diff) <= 1, diff
    for i in diff:
        P = ref.process(tl[i], c.proc, exact=True).double().numpy()
        Q = ref.process(dl[i], c.proc, exact=True).double().numpy()
        r = tref.philox_step(P, Q, tok[i].numpy(), parent, mw.SEED, mw.OFFSET, 3 + i, stops, greedy=not c.proc.stochastic)
        cc = SimpleNamespace(proc=c.proc, dtype=dtype, tl=tl, dl=dl)
        check_draw(f"row {i}", r, int(got.next_token[i]), tw.draw_slack(cc, i, r))


# ---------------------------------------------------------------- losslessness on the device
def _context_free(n_rows, V, dtype, seed, tail=False):
    g = torch.Generator().manual_seed(seed)
    tl = torch.randn(n_rows, V, generator=g) * 2
    noise = 0.8 * torch.randn(n_rows, V, generator=g)
    if tail:                                                          # as multi_walk.edge_case: +8 / +6
        tl[:, mw.last_chunk_start(V):] += 8
        noise[:, mw.last_chunk_start(V):] -= 2
    tl = tl.to(dtype)
    dl = (tl.float() + noise).to(dtype)
    proc = mw.PROCS["multinomial"]
    return tl, dl, ref.process(tl, proc, exact=True).double().numpy(), ref.process(dl, proc, exact=True).double().numpy()


@pytest.mark.parametrize("V", [64, 1000, 4101])
def test_first_token_keeps_the_target_distribution(sd, V):
    """from_branching([4]): 4096 sequences with identical rows, the children iid from the exact q on
    the host; the first emitted token over the batch against the exact processed p (V = 4101: three
    chunks with the boosted tail)."""
    B, parent = 4096, tw.from_branching([4])
    tl, dl, p, q = _context_free(2, V, torch.bfloat16, 5, tail=V > tw.CHUNK)
    rng = np.random.default_rng(104)
    tok = torch.from_numpy(rng.choice(V, size=(B, 4), p=q[0] / q[0].sum()))
    T = torch.stack([tl[0]] + [tl[1]] * 4).to(DEV).expand(B, 5, V).contiguous()
    D = dl[:1].to(DEV).expand(B, 1, V).contiguous()
    out = sd.ops.verify_tree(T, D, tok.to(DEV), parent, spec_of(sd, mw.PROCS["multinomial"]), sd.PhiloxNoise(seed=99, offset=3),
                             pad_token_id=PAD)
    first = out.tokens_out[:, 0].cpu().numpy()
    assert first.min() >= 0
    st = out.row_status.cpu().numpy()
    assert (st & sd.lib.SD_ROW_RESIDUAL != 0).sum() > 0 and (st & sd.lib.SD_ROW_BONUS != 0).sum() > B // 32
    chi2_check(first, p[0], f"tree [4] first token V={V}")


@pytest.mark.parametrize("V", [64, 1000, 4101])
def test_two_tokens_keep_the_target_distribution(sd, V):
    """from_branching([2, 2]) with context-dependent rows: each depth-1 node has its own target and
    drafter row.  The first emitted token against the exact p of the root; the second, over the
    sequences whose first token is the most frequent one a, against p(· | a) — the target row of the
    node that drafted a (both root children draw from the same q, and every node that holds token a
    gets the rows of context a, as a model would give them)."""
    B, parent = 4096, tw.from_branching([2, 2])
    tl, dl, p, q = _context_free(1 + V, V, torch.bfloat16, 7, tail=V > tw.CHUNK)     # row 0: the root; row 1 + a: context a
    rng = np.random.default_rng(222)
    t0 = rng.choice(V, size=(B, 2), p=q[0] / q[0].sum())
    t1 = np.stack([rng.choice(V, p=q[1 + t0[b, k]] / q[1 + t0[b, k]].sum(), size=2) for b in range(B) for k in range(2)]
                  ).reshape(B, 4)
    tok = torch.from_numpy(np.concatenate([t0, t1], 1))
    tld, dld = tl.to(DEV), dl.to(DEV)
    ctx = torch.from_numpy(1 + t0).to(DEV)                                            # rows of the two depth-1 slots
    T = torch.empty(B, 7, V, dtype=tl.dtype, device=DEV)
    T[:, 0] = tld[0]
    T[:, 1:3] = tld[ctx]
    # the leaves' rows: context (a, b) gets row 1 + (a + b) % V — any fixed function of the path serves
    leaf_ctx = 1 + (torch.from_numpy(t0).to(DEV).repeat_interleave(2, 1) + tok[:, 2:].to(DEV)) % V
    T[:, 3:7] = tld[leaf_ctx]
    D = torch.stack([dld[0].expand(B, V), dld[ctx[:, 0]], dld[ctx[:, 1]]], 1).contiguous()
    out = sd.ops.verify_tree(T, D, tok.to(DEV), parent, spec_of(sd, mw.PROCS["multinomial"]), sd.PhiloxNoise(seed=77, offset=9),
                             pad_token_id=PAD)
    toks = out.tokens_out.cpu().numpy()
    first = toks[:, 0]
    assert first.min() >= 0
    chi2_check(first, p[0], f"tree [2,2] first token V={V}")
    # second token given the first: only where the first was an accepted draft does a second exist
    n = out.n_accepted.cpu().numpy()
    a = int(np.bincount(first[n >= 1]).argmax())
    sel = (n >= 1) & (first == a)
    assert sel.sum() >= 50, sel.sum()            # chi2_check pools the bins that expect fewer than 5
    chi2_check(toks[sel, 1], p[1 + a], f"tree [2,2] second token given {a} V={V}")


# ---------------------------------------------------------------- stop lists
@pytest.mark.parametrize("n_stop", [1, 64])
def test_stop_on_the_accepted_path(sd, n_stop):
    c = tw.case(33, "b4211", 2049, torch.bfloat16, "multinomial", True)
    free = tw.host_results(c)
    b_hit = next(b for b, r in enumerate(free) if r.n >= 2)
    r = free[b_hit]
    stop = int(c.tok[b_hit, r.path[r.n - 1]])
    first = int(c.tok[b_hit, r.path[0]])
    filler = [c.V + 10 + i for i in range(n_stop - 1)]                # ids no draft holds
    stops = filler + [stop] + ([first] if n_stop > 1 else [])         # listed later: the earlier-listed stop wins
    rows = tw.host_results(c, stops)
    assert rows[b_hit].status == tref.STOP and rows[b_hit].stop_index >= 0
    got = run_tree(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.parent, c.proc, tw.SEED, tw.OFFSET, tw.ROW_BASE, stops)
    check_case(sd, c, got, rows)
    assert int(got.row_status[b_hit]) & sd.lib.SD_ROW_STOP_IN_DRAFTS and int(got.next_token[b_hit]) == -1


# ---------------------------------------------------------------- one workspace, many entry points
def test_one_workspace_serves_changing_shapes_and_entry_points(sd):
    shapes = [(33, "b4211", 2049, torch.bfloat16, "multinomial", True), (1, "irregular64", 64, torch.float32, "topk50"),
              (33, "fan8", 4097, torch.float16, "multinomial_T0.7", True)]
    cases = [tw.case(*s) for s in shapes]
    run = lambda c: run_tree(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.parent, c.proc, tw.SEED, tw.OFFSET,  # noqa: E731
                             tw.ROW_BASE)
    first = [run(c) for c in cases]
    spec = sd.ops.ProcSpec("multinomial", 1.0)
    m = mw.case(3, 3, 5, 1000, torch.bfloat16, "topk50")
    blogits = (torch.randn(4, 4096, generator=torch.Generator().manual_seed(3)) * 3).to(torch.bfloat16).to(DEV)
    for rnd in range(2):
        for c, want in zip(cases, first):
            x = c.tl.to(DEV)
            sd.ops.verify([x[:, 0], x[:, 1]], [c.dl[:, 0].to(DEV)], c.tok[:, :1].contiguous().to(DEV), sd.lib.SD_RULE_SPEC,
                          spec, spec, sd.PhiloxNoise(seed=1, offset=rnd))
            sd.ops.sample_rows(x[:, 0].contiguous(), spec, sd.PhiloxNoise(seed=2, offset=rnd))
            sd.ops.verify_multi(m.tl.to(DEV), m.dl.to(DEV), m.tok.to(DEV), spec_of(sd, m.proc),
                                sd.PhiloxNoise(seed=3, offset=rnd))
            beam = sd.ops.BeamState.start([3, 4, 5, 6], 4, 16, 0, DEV)          # a whole beam step: row pass + selection
            beam.probs[:, 4:6] = -1.0
            sd.ops.beam_step(beam, blogits[:, :min(c.V, 4096)].contiguous(), 6, top_k=3, length=2, pad_token_id=0)
            again = run(c)
            for f in FIELDS:
                a, w = getattr(again, f), getattr(want, f)
                if f == "resample_mass":
                    a, w = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(w, nan=-1.0)
                assert torch.equal(a, w), f


# ---------------------------------------------------------------- graph capture
def test_capture_and_replay_with_an_advanced_offset(sd):
    c = tw.case(33, "b4211", 2049, torch.bfloat16, "multinomial", True)
    tree = sd.TokenTree(c.parent)
    tl, dl, tok = c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV)
    draft = dl[:, tree.internal_slots].contiguous()
    spec = spec_of(sd, c.proc)
    off = torch.tensor([tw.OFFSET], dtype=torch.long, device=DEV)
    noise = sd.PhiloxNoise(seed=tw.SEED, offset=0, offset_dev=off)   # the eager call takes host offset 0, the captured one 1
    eager = sd.ops.verify_tree(tl, draft, tok, tree, spec, noise, row_base=tw.ROW_BASE, pad_token_id=PAD)   # sizes the workspace
    want0 = {f: getattr(eager, f).clone() for f in FIELDS}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sd.ops.verify_tree(tl, draft, tok, tree, spec, noise, row_base=tw.ROW_BASE, pad_token_id=PAD)
    off.fill_(tw.OFFSET + 5)
    graph.replay()
    torch.cuda.synchronize()
    got = SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})
    check_case(sd, c, got, tw.host_results(c, off=1 + tw.OFFSET + 5))
    assert not all(torch.equal(torch.nan_to_num(getattr(got, f).float(), nan=-1.0),
                               torch.nan_to_num(want0[f].cpu().float(), nan=-1.0)) for f in FIELDS)


# ---------------------------------------------------------------- row layouts, -inf entries
@pytest.mark.parametrize("layout", rowe.LAYOUTS)
@pytest.mark.parametrize("V,dtype,name,mask", [(2047, torch.bfloat16, "multinomial", "none"), (65, torch.float32, "topk50", "half"),
                                               (2049, torch.float16, "greedy", "half"), (9, torch.bfloat16, "nucleus0.9", "most")])
def test_rows_in_a_poisoned_buffer(sd, layout, V, dtype, name, mask):
    """Padded, shifted and packed (16-byte-misaligned where V * itemsize % 16 != 0) rows inside a
    buffer of +inf / NaN: an element outside a row that reaches a sum, a maximum or a draw shows as a
    wrong or flagged row.  Rows with `-inf` entries (mask) run through the same cases."""
    c = tw.case(33, "b4211", V, dtype, name, False, mask)
    tree = sd.TokenTree(c.parent)
    poison = rowe.poison_of(layout, V, name)
    tl = rowe.place(c.tl, layout, poison, DEV)
    dl = rowe.place(c.dl[:, tree.internal_slots].contiguous(), layout, poison, DEV)
    out = sd.ops.verify_tree(tl, dl, c.tok.to(DEV), tree, spec_of(sd, c.proc), sd.PhiloxNoise(seed=tw.SEED, offset=tw.OFFSET),
                             row_base=tw.ROW_BASE, pad_token_id=PAD)
    got = SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})
    check_case(sd, c, got, tw.host_results(c))


# ---------------------------------------------------------------- out-of-range draft ids
def test_out_of_range_ids_as_sd_verify_multi(sd):
    """Ids outside [0, V) at a root child and at a deeper node: the same n, rejects, status and token
    as sd_verify_multi gives on the equivalent chains (p = q = 0 there: the test accepts, as SPEC)."""
    K, g = 2, 3
    c0 = mw.case(16, K, g, 4096, torch.bfloat16, "multinomial")
    tl_m, dl_m = _same_root_rows(c0)
    tokm = c0.tok.clone()
    tokm[:, 0, 0] = 4096 + torch.arange(16)          # chain 0's first draft: beyond V (distinct from chain 1's)
    tokm[::2, 0, 1] = -3                             # chain 0's second draft on even rows: negative
    c = SimpleNamespace(**{**vars(c0), "tl": tl_m, "dl": dl_m, "tok": tokm})
    bs = list(range(16))
    multi = sd.ops.verify_multi(tl_m.to(DEV), dl_m.to(DEV), tokm.to(DEV), spec_of(sd, c.proc),
                                sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET), row_base=3)
    tl, dl, tok = _chain_tree_inputs(c, bs)
    got = run_tree(sd, tl.to(DEV), dl.to(DEV), tok.to(DEV), tw.chains(K, g), c.proc, mw.SEED, mw.OFFSET, 3)
    assert torch.equal(got.n_accepted, multi.n_accepted.cpu())
    assert torch.equal(got.n_sibling_rejects, multi.n_sibling_rejects.cpu())
    assert torch.equal(got.row_status, multi.row_status.cpu())
    assert int((got.next_token != multi.next_token.cpu()).sum()) <= 1
    assert int((got.n_accepted >= 1).sum()) == 16     # the out-of-range root child is accepted everywhere
    assert int((got.n_accepted[::2] >= 2).sum()) == 8  # and the negative id below it


# ---------------------------------------------------------------- the dispatcher-visible operator
def test_torch_op_equals_ops_verify_tree(sd):
    c = tw.case(33, "b4211", 2049, torch.bfloat16, "multinomial", True)
    tree = sd.TokenTree(c.parent)
    tl, dl, tok = c.tl.to(DEV), c.dl[:, tree.internal_slots].contiguous().to(DEV), c.tok.to(DEV)
    stops = torch.tensor([int(c.tok[2, 0])], dtype=torch.long, device=DEV)
    want = sd.ops.verify_tree(tl, dl, tok, tree, spec_of(sd, c.proc), sd.PhiloxNoise(seed=tw.SEED, offset=tw.OFFSET),
                              stop_tokens=stops, row_base=tw.ROW_BASE)
    got = torch.ops.specdec.verify_tree(tl, dl, tok, c.parent, stops, sd.ops.KIND[c.proc.kind], c.proc.temperature,
                                        c.proc.top_k, c.proc.top_p, tw.SEED, tw.OFFSET, tw.ROW_BASE)
    for g, f in zip(got, sd.ops.TREE_FIELDS + ("path",)):
        w = getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, f
        assert torch.equal(torch.nan_to_num(g.float(), nan=-1.0), torch.nan_to_num(w.float(), nan=-1.0)), f
