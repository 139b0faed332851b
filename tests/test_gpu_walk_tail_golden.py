"""The multi-draft, token-tree, distinct-children, dynamic-tree and vocabulary-parallel verifies share one
definition of their tail (csrc/sd_pick.h: chunk pick, in-chunk pick, greedy reduction; the stop scan, the row
constructor and the trees' output block beside it).  Sharing it changed no arithmetic and no order of
summation, so every output keeps its bits: this file holds the library to what the commit BEFORE the
change returned for the same calls (tests/golden/walk_tail.json, written by tests/golden/make_walk_tail.py
with that commit's build), integer outputs as integers and resample_mass by its bit pattern.

Cases (all inputs from seeds, built by the existing case builders):
  vocabulary   5 (less than one vector), 2048 (exactly one chunk), 2049 (a second chunk of one element),
               4097 (a ragged third chunk); above one chunk the short last chunk is boosted, so draws land in it
  processor    multinomial, multinomial at T = 0.7, greedy, top-k 50 (vocabulary-parallel: the first three)
  dtype        bf16, fp32 (the vector widths differ), alternating over the (vocabulary, processor) grid so
               that every vocabulary and every processor meets both
  multi-draft  (K, γ) in (1, 1), (2, 3), (4, 4), cycling over the grid (multi_walk.edge_case)
  trees        a 3-wide fan, chains(2, 2), [-1, -1, 0, 0, 1], cycling (tree_walk.case for sd_verify_tree,
               tree_distinct_walk.case for the distinct form, both given the parent list)
  dynamic      tree_dynamic_cases.case's grown trees: a topology and its tokens per sequence (3 sequences, 7
               nodes, depth 2), a fourth sequence with an invalid parent list; target rows from a seed, with the
               first child of every slot at nearly all the mass (sequence 0) or lifted (2), every child lowered (1)
  vp           two shards of 2049 elements (vp_cases.case), γ' = 3
  batch        multi / tree / distinct: one call of 3 sequences (the scenarios that leave the drafts, reject at
               the root and reject below it: residual exits) and one call of 1 sequence, the scenario that
               accepts down to a bonus exit (multi "full", tree "last", distinct "first"), at its own global
               row; dynamic 4; vp 1 and 3
  stops        none; and, for the one-sequence calls, the dynamic batches and the 3-sequence vp calls, where a
               sequence accepted two different tokens, the list (second, first): the entry listed first occurs
               later on the path than the second and must still win (stop_index 1).  Every path has such a call.
The stop lists depend on what was accepted, so the fixture records them; the test reads them from there.
"""
import json
import os
from types import SimpleNamespace

import pytest
import torch

import multi_walk as mw
import tree_distinct_walk as dw
import tree_dynamic_cases as ydc
import tree_walk as tw
import vp_cases as vc
from tree_ref import children_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_tail.json")

VOCABS = (5, 2048, 2049, 4097)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
PROC_NAMES = ("multinomial", "multinomial_T0.7", "greedy", "topk50")
MULTI_SHAPES = ((1, 1), (2, 3), (4, 4))
TREES = {"fan3": tuple(tw.from_branching([3])), "chains22": tuple(tw.chains(2, 2)), "five": (-1, -1, 0, 0, 1)}
GRID = [(V, list(DTYPES)[(i + j) % 2], name) for i, V in enumerate(VOCABS) for j, name in enumerate(PROC_NAMES)]
BONUS_SEQ = {"multi": 4, "tree": 3, "distinct": 3}     # the sequence (scenario) of the one-sequence call
PATHS = ("multi", "tree", "distinct", "dynamic", "vp")
MULTI_FIELDS = ("n_accepted", "winner", "next_token", "resample_mass", "n_sibling_rejects", "prune_drafter", "prune_target",
                "stop_index", "row_status", "tokens_out")
TREE_FIELDS = ("n_accepted", "last_node", "next_token", "resample_mass", "n_sibling_rejects", "stop_index", "row_status", "path",
               "tokens_out")
VP_FIELDS = ("n_accepted", "next_token", "resample_mass", "prune_drafter", "prune_target", "stop_index", "row_status",
             "owner_shard")


def lib():
    from specdec_amd import _lib, ops, vocab_parallel
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    return SimpleNamespace(lib=_lib, ops=ops, vp=vocab_parallel, PhiloxNoise=PhiloxNoise, TokenTree=TokenTree)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def record(out, fields):
    """{field: list of integers} (fp32: the bit patterns)."""
    rec = {}
    for f in fields:
        t = getattr(out, f).cpu()
        rec[f] = (t.view(torch.int32) if t.dtype == torch.float32 else t).flatten().tolist()
    return rec


def flat(rec, fields):
    """What the fixture stores of a record: the fields' integers in the fields' order."""
    return [x for f in fields for x in rec[f]]


def stop_tensor(stops):
    return torch.tensor(list(stops), dtype=torch.long, device=DEV)


def dynamic_inputs(V, dt):
    """(tl [4, 8, V], tok [4, 7], parents [4][7]): the trees tree_dynamic_cases grows for 3 sequences and,
    fourth, sequence 0's tokens under a parent list whose node 2 is its own parent."""
    c = ydc.case(V, 3, 2, 3, 2, 7, DTYPES[dt])
    parents = [list(m.sel.parent) for m in c.models] + [[-1, -1, 2, 0, 0, 1, 1]]
    tok = torch.tensor([list(m.sel.tokens) for m in c.models] + [list(c.models[0].sel.tokens)])
    tl = torch.randn(4, 8, V, generator=torch.Generator().manual_seed(1000 * V + c.seed)) * 3
    for b in range(3):
        for s, cs in enumerate(children_of(parents[b])):
            if cs and b == 1:
                tl[b, s, tok[b, cs]] -= 12
            elif cs and b == 2:
                tl[b, s, tok[b, cs[0]]] += 10
            elif cs:
                tl[b, s, tok[b, cs[0]]] = 20.0          # nearly all the row's mass: the walk goes down to a leaf
    return tl.to(DTYPES[dt]), tok, parents


def calls():
    """{id: (fields, run, with_stops)}; run(sd, stops) makes the call and returns (its outputs, a tensor
    [B, >= n] whose row b starts with sequence b's accepted tokens); with_stops: the call is repeated
    with a swapped stop list."""
    out = {}
    for n, (V, dt, name) in enumerate(GRID):
        K, g = MULTI_SHAPES[n % 3]
        tname = list(TREES)[n % 3]
        for part, sl in (("3", slice(0, 3)), ("1", None)):
            def multi(sd, stops, K=K, g=g, V=V, dt=dt, name=name, sl=sl):
                c = mw.edge_case(5, K, g, V, DTYPES[dt], name, V > mw.CHUNK)
                s = sl or slice(BONUS_SEQ["multi"], BONUS_SEQ["multi"] + 1)
                o = sd.ops.verify_multi(c.tl[s].to(DEV), c.dl[s].to(DEV), c.tok[s].to(DEV), spec_of(sd, c.proc),
                                        sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET), stop_tokens=stop_tensor(stops),
                                        row_base=mw.ROW_BASE + s.start, pad_token_id=PAD)
                return o, o.tokens_out

            def tree(sd, stops, tname=tname, V=V, dt=dt, name=name, sl=sl):
                c = tw.case(1, TREES[tname], V, DTYPES[dt], name, V > tw.CHUNK)
                s = sl or slice(BONUS_SEQ["tree"], BONUS_SEQ["tree"] + 1)
                t = sd.TokenTree(c.parent)
                draft = [c.dl[s, i].to(DEV) if t.children[i] else None for i in range(t.num_nodes + 1)]
                o = sd.ops.verify_tree(c.tl[s].to(DEV), draft, c.tok[s].to(DEV), t, spec_of(sd, c.proc),
                                       sd.PhiloxNoise(seed=tw.SEED, offset=tw.OFFSET), stop_tokens=stop_tensor(stops),
                                       row_base=tw.ROW_BASE + s.start, pad_token_id=PAD)
                return o, o.tokens_out

            def distinct(sd, stops, tname=tname, V=V, dt=dt, name=name, sl=sl):
                c = dw.case(TREES[tname], V, DTYPES[dt], name)
                s = sl or slice(BONUS_SEQ["distinct"], BONUS_SEQ["distinct"] + 1)
                o = sd.ops.verify_tree_distinct(c.tl[s].to(DEV), c.tok[s].contiguous().to(DEV), sd.TokenTree(c.parent),
                                                spec_of(sd, c.proc), sd.PhiloxNoise(seed=dw.SEED, offset=dw.OFFSET),
                                                stop_tokens=stop_tensor(stops), pad_token_id=PAD, row_base=dw.ROW_BASE + s.start)
                return o, o.tokens_out

            tag = f"V{V}-{dt}-{name.replace('multinomial', 'mn')}/{part}"
            out[f"multi/K{K}g{g}-{tag}"] = (MULTI_FIELDS, multi, sl is None)
            out[f"tree/{tname}-{tag}"] = (TREE_FIELDS, tree, sl is None)
            out[f"distinct/{tname}-{tag}"] = (TREE_FIELDS, distinct, sl is None)
    for V, dt, name in ((2048, "bf16", "multinomial"), (2049, "fp32", "multinomial_T0.7"), (4097, "bf16", "greedy"),
                        (4097, "fp32", "topk50")):
        def dynamic(sd, stops, V=V, dt=dt, name=name):
            tl, tok, parents = dynamic_inputs(V, dt)
            o = sd.ops.verify_tree_dynamic(tl.to(DEV), tok.to(DEV), torch.tensor(parents, dtype=torch.int32, device=DEV),
                                           spec_of(sd, mw.PROCS[name]), sd.PhiloxNoise(seed=dw.SEED, offset=dw.OFFSET), 2,
                                           stop_tokens=stop_tensor(stops), pad_token_id=PAD, row_base=dw.ROW_BASE)
            return o, o.tokens_out

        out[f"dynamic/V{V}-{dt}-{name.replace('multinomial', 'mn')}/4"] = (TREE_FIELDS, dynamic, True)
    n = 0
    for B in (1, 3):
        for dt in DTYPES:
            for name in PROC_NAMES[:3]:
                def vp(sd, stops, B=B, dt=dt, name=name, own=n % 2 == 1):
                    c = vc.case(B, 3, 4098, (2049, 2049), DTYPES[dt], name, False, own)
                    ls = sd.vp.LocalShards(sd.vp.VocabShard.split(c.sizes))
                    outs = sd.vp.verify_vocab_parallel(c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), spec_of(sd, c.proc),
                                                       sd.PhiloxNoise(seed=vc.SEED, offset=vc.OFFSET), None, ls,
                                                       stop_tokens=stop_tensor(stops or c.stops), row_base=vc.ROW_BASE)
                    return outs[0], c.tok

                out[f"vp/B{B}-{dt}-{name.replace('multinomial', 'mn')}" + ("-stop" if n % 2 else "")] = (VP_FIELDS, vp, B == 3)
                n += 1
    return out


def swapped_stops(rec, toks):
    """(sequence b, [second, first accepted token of b]) for the first sequence that accepted two different
    tokens, or None."""
    for b, n in enumerate(rec["n_accepted"]):
        if n >= 2 and int(toks[b, 0]) != int(toks[b, 1]):
            return b, [int(toks[b, 1]), int(toks[b, 0])]
    return None


def run_all(sd, golden=None):
    """{id: {"out": record, and with a stop list "stops", "hit" (the sequence it was made from), "out_stops"}};
    with `golden`, the stop lists come from it (else from this run's own outputs)."""
    got = {}
    for cid, (fields, run, with_stops) in calls().items():
        o, toks = run(sd, ())
        got[cid] = {"out": record(o, fields)}
        if with_stops:
            if golden is None:
                s = swapped_stops(got[cid]["out"], toks.cpu())
            else:
                s = (golden[cid]["hit"], golden[cid]["stops"]) if "stops" in golden[cid] else None
            if s:
                got[cid].update(hit=s[0], stops=s[1], out_stops=record(run(sd, s[1])[0], fields))
    torch.cuda.synchronize()
    return got


def stored(got):
    """The fixture's form of run_all's result: records flattened."""
    fields = {cid: f for cid, (f, _, _) in calls().items()}
    return {cid: {k: (flat(v, fields[cid]) if k in ("out", "out_stops") else v) for k, v in e.items()} for cid, e in got.items()}


def stop_hits(got):
    """Per path, the calls whose swapped stop list ended the sequence at position 1."""
    return {p: [c for c, e in got.items() if c.startswith(p + "/") and "stops" in e and e["out_stops"]["stop_index"][e["hit"]] == 1]
            for p in PATHS}


def test_every_output_keeps_the_parent_commits_bits():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = run_all(lib(), golden)
    assert sorted(got) == sorted(golden)
    hits = stop_hits(got)
    assert all(hits[p] for p in PATHS), hits              # every path: the listed-first stop, met later, wins
    mine = stored(got)
    bad = [(c, k) for c in golden for k in golden[c] if mine[c].get(k) != golden[c][k]]
    n_seq = sum(len(e[k]["n_accepted"]) for e in got.values() for k in ("out", "out_stops") if k in e)
    print(f"[walk-tail] {len(golden)} calls, {n_seq} sequences, {len(bad)} records differ")
    assert not bad, [(c, k, mine[c].get(k), golden[c][k]) for c, k in bad[:5]]
