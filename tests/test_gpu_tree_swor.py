"""sd_verify_tree_swor (csrc/sd_verify_tree_swor.inc): walks against the fp64 host model under tests/test_gpu_tree.py's
conventions (at most one row per case may differ, and only a close one: tests/test_tree_swor_cpu.py asserts the cap),
one-child trees against sd_verify_tree, sample_distinct + verify_tree_swor end to end, graph capture, the loop."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_tree as tg
import tree_ref as tref
import tree_swor_ref as sw
import tree_walk as tw
from test_gpu_tree import sd  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
TREES = {"b4": tw.from_branching([4]), "b321": tw.from_branching([3, 2, 1]), "irregular64": tw.TREES["irregular64"]}
DRAW_OFFSET = 91                                       # the children's Gumbel noise: another offset than the walk's
# (tree, V, dtype, processor, variant): the full product, then a duplicated, a -1 and an out-of-range sibling
WALKS = [(t, V, dt, name, "drawn") for t in TREES for V in [64, 2049, 4101] for dt in (torch.bfloat16, torch.float32)
         for name in ("multinomial", "nucleus0.9")]
WALKS += [("b321", 2049, torch.bfloat16, "multinomial", v) for v in ("duplicate", "minus_one", "out_of_range")]


@functools.lru_cache(maxsize=None)
def host_walk(tname, V, dtype, name, variant):
    """(case, host rows): tests/tree_walk.py's rows, 8 sequences, their children drawn by the host model."""
    c = tw.case(8, tuple(TREES[tname]), V, dtype, name)
    Q = c.Q.double().numpy()
    tok = torch.from_numpy(np.stack([sw.draw_children(Q[b], c.parent, tw.SEED, DRAW_OFFSET, lambda s, b=b: b * (c.N + 1) + s)
                                     for b in range(c.B)]))
    if variant != "drawn":                             # the root's second child, on every sequence
        tok[:, 1] = {"duplicate": tok[:, 0], "minus_one": -1, "out_of_range": V + 3}[variant]
    c = SimpleNamespace(**{**vars(c), "tok": tok})
    return c, [sw.under_rule(tref.philox_step, c.P[b].double().numpy(), Q[b], tok[b].numpy(), c.parent, tw.SEED, tw.OFFSET,
                             tw.ROW_BASE + b) for b in range(c.B)]


def run(sd, fn, c):
    tree = sd.TokenTree(c.parent)
    out = fn(c.tl.to(tg.DEV), c.dl[:, tree.internal_slots].contiguous().to(tg.DEV), c.tok.to(tg.DEV), tree, tg.spec_of(sd, c.proc),
             sd.PhiloxNoise(seed=tw.SEED, offset=tw.OFFSET), row_base=tw.ROW_BASE, pad_token_id=tg.PAD)
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in tg.FIELDS})


@pytest.mark.parametrize("case", WALKS, ids=lambda c: f"{c[0]}-V{c[1]}-{str(c[2]).split('.')[-1]}-{c[3]}-{c[4]}")
def test_walks_equal_the_host_model(sd, case):
    c, rows = host_walk(*case)
    got = run(sd, sd.ops.verify_tree_swor, c)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_TREE_SWOR
    tg.check_case(sd, c, got, rows)
    if case[4] != "drawn":                             # some walk met the weightless sibling (recorded with a NaN ratio)
        assert any(t[2] != t[2] for r in rows for t in r.tests)


@pytest.mark.parametrize("g", [1, 5])
def test_one_child_trees_equal_sd_verify_tree_bit_for_bit(sd, g):
    c = tw.case(33, tuple(tw.chains(1, g)), 2049, torch.bfloat16, "multinomial")
    want, got = run(sd, sd.ops.verify_tree, c), run(sd, sd.ops.verify_tree_swor, c)
    assert all(torch.equal(getattr(got, f).view(torch.uint8), getattr(want, f).view(torch.uint8)) for f in tg.FIELDS)


@pytest.mark.parametrize("V", [64, 4101])
@pytest.mark.parametrize("widths", [(4,), (2, 2)], ids=["b4", "b22"])
def test_draw_and_verify_keep_the_target_distribution(sd, V, widths):
    """4096 sequences, context-dependent rows (row 0: the root's, row 1 + a: context a), children from sample_distinct
    (slabs of 64 rows, global row = the row's index): the first emitted token against the exact p, the second, given
    the most frequent accepted first token a, against p(. | a).  A draw whose weights were not the verify's q fails."""
    from test_gpu_perfmode import chi2_check
    B, c, spec = 4096, widths[0], sd.ops.ProcSpec("multinomial", 1.0)
    tl, dl, p, _ = tg._context_free(1 + V, V, torch.bfloat16, 7, tail=V > tw.CHUNK)
    tl, dl = tl.to(tg.DEV), dl.to(tg.DEV)

    def draw(at, k, off):                              # at: the rows' indices into dl
        return torch.cat([sd.ops.sample_distinct(dl[at[r0:r0 + 64]], k, spec, sd.PhiloxNoise(seed=41, offset=off), row_base=r0)[0]
                          for r0 in range(0, len(at), 64)])

    t0 = draw(torch.zeros(B, dtype=torch.long, device=tg.DEV), c, 1)                   # [B, c]
    T, D, tok = [tl[:1].expand(B, V), *tl[1 + t0].unbind(1)], dl[:1].expand(B, 1, V), t0
    if len(widths) == 2:
        t1 = draw((1 + t0).reshape(-1), widths[1], 2).reshape(B, -1)                # [B, c * widths[1]]
        T += tl[1 + (t0.repeat_interleave(widths[1], 1) + t1) % V].unbind(1)        # leaves: any fixed function of the path
        D, tok = torch.cat([D, dl[1 + t0]], 1), torch.cat([t0, t1], 1)
    out = sd.ops.verify_tree_swor(torch.stack(T, 1), D.contiguous(), tok, tw.from_branching(list(widths)), spec,
                                  sd.PhiloxNoise(seed=77, offset=9), pad_token_id=tg.PAD)
    emitted, n = out.tokens_out.cpu().numpy(), out.n_accepted.cpu().numpy()
    first = emitted[:, 0]
    assert first.min() >= 0 and not int(out.row_status.cpu().numpy().max()) & sd.lib.SD_ROW_ERROR_MASK
    chi2_check(first, p[0], f"swor {widths} first token V={V}")
    if len(widths) == 2:
        a = int(np.bincount(first[n >= 1]).argmax())
        sel = (n >= 1) & (first == a)
        assert sel.sum() >= 50, sel.sum()
        chi2_check(emitted[sel, 1], p[1 + a], f"swor {widths} second token given {a} V={V}")


def test_a_captured_draw_and_verify_pair_replays_bit_for_bit(sd):
    c = tw.case(33, tuple(TREES["b4"]), 2049, torch.bfloat16, "multinomial")
    tl, dl, spec = c.tl.to(tg.DEV), c.dl[:, :1].contiguous().to(tg.DEV), tg.spec_of(sd, c.proc)

    def pair():
        tok, _ = sd.ops.sample_distinct(dl[:, 0], 4, spec, sd.PhiloxNoise(seed=5, offset=1))
        out = sd.ops.verify_tree_swor(tl, dl, tok, c.parent, spec, sd.PhiloxNoise(seed=5, offset=2), pad_token_id=tg.PAD)
        return [tok] + [getattr(out, f) for f in tg.FIELDS]

    want = [t.clone() for t in pair()]                 # eager: sizes the workspace too
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = pair()
    for _ in range(3):
        [t.zero_() for t in outs]
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(g.view(torch.uint8), w.view(torch.uint8)) for g, w in zip(outs, want))


def test_the_cached_distinct_loops_emit_the_uncached_loops_tokens():
    """The fp32 test Llama pair: every cached loop emits the uncached loop's tokens; GreedyProcessor raises ValueError."""
    import test_gpu_tree_cached_loop as tc
    pytest.importorskip("transformers")
    target = tc._tiny_llama(1).to(tg.DEV)
    models, trace = (target, tc._tiny_llama(2, noise_of=target).to(tg.DEV)), []
    want = tc._generate(*models, "b221", "multinomial", children="distinct", trace=trace)
    assert len(want[0]) == tc.GEN and 0 < sum(s["n"] for s in trace)
    assert all(len(set(s["draft_tokens"][:2].tolist())) == 2 for s in trace if s["draft_tokens"].numel() >= 2)   # distinct siblings
    for kw in [*tc.KINDS.values(), dict(use_cache=True, attention="kernel")]:
        assert tc._generate(*models, "b221", "multinomial", children="distinct", **kw) == want, kw
    with pytest.raises(ValueError, match='children="topk"'):
        tc._generate(*models, "b221", "greedy", children="distinct")
