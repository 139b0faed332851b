"""What the dynamic draft trees cost: one growth level, the per-sequence verify, and the loop.

    python scripts/tree_dynamic_timing.py [--steps 200] [--trials 5] [--skip-loop] [--out FILE]      (GPU)

All at B = 1, V = 128256, bf16; device events around blocks of calls that alternate in one process after a
warm-up; the median of the trials (microseconds per call).

1. One growth level (sd_tree_grow, level 3 of (W, c) = (8, 8): 8 frontier rows, 64 candidates, the 8 best
   kept) against the torch expression of the same level on the device — log_softmax + topk + add + topk +
   gathers.  The torch expression is the yardstick, not the code under test.
2. sd_verify_tree_dynamic against sd_verify_tree_distinct (the parent commit's code) on the same topology
   and rows, from_branching([4,2,1,1]) and the irregular 64-node tree, multinomial and greedy.  The margin
   the dynamic call gets is the yardstick's own max / min spread over its trials.
3. dynamic_tree_speculative_generate against tree_speculative_generate(children="topk",
   tree=from_branching([4,2,1,1])), both uncached, N = 28 nodes per target forward, on the random-init
   Llama-3.2-1B-shaped target and 4-layer drafter of scripts/kv_compact_timing.py: accepted tokens per
   target forward and tokens per second.  Random-init models say little about real acceptance.

Writes profiles/tree_dynamic_timing.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

VOCAB, DEV = 128256, "cuda"


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def alternate(calls, steps, trials):
    for _ in range(20):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(trials):
        for k, fn in calls.items():
            us[k].append(round(timed(fn, steps), 2))
    return us, {k: statistics.median(v) for k, v in us.items()}


def grow_table(steps, trials):
    from specdec_amd import ops
    from specdec_amd.tree import DynamicTreeSpec
    W = c = 8
    sp = DynamicTreeSpec(3, W, c, 64)
    g = torch.Generator().manual_seed(1)
    pool = ops.tree_pool(1, sp.pool_size, DEV)
    rows = [(torch.randn(1, F, VOCAB, generator=g) * 3).to(torch.bfloat16).to(DEV) for F in sp.frontier[:3]]
    f1 = ops.tree_grow(rows[0], 1, W, c, pool)
    f2 = ops.tree_grow(rows[1], 2, W, c, pool, f1.pool)
    x, fin = rows[2], f2.pool.clone()
    base = sp.base[2]

    def torch_level():
        lp = torch.log_softmax(x[0].float(), -1)                       # fp32 log-probabilities, as the kernel's
        top = torch.topk(lp, c, dim=-1)
        pscore = pool.score[0].gather(0, fin[0].long())
        score = (pscore[:, None] + top.values).reshape(-1)
        keep = torch.topk(score, W).indices.sort().values
        return top.indices.reshape(-1).gather(0, keep), keep + base, keep // c, score

    calls = {"tree_grow": lambda: ops.tree_grow(x, 3, W, c, pool, fin), "torch": torch_level}
    got, want = calls["tree_grow"](), torch_level()
    same = bool(torch.equal(got.token[0], want[0]) and torch.equal(got.pool[0].long(), want[1]))
    us, med = alternate(calls, steps, trials)
    rec = dict(level=3, width=W, branch=c, frontier_rows=8, vocab=VOCAB, dtype="bf16", same_frontier_as_torch=same,
               trials_us=us, median_us=med, ratio_grow_over_torch=round(med["tree_grow"] / med["torch"], 3))
    print(json.dumps(rec), flush=True)
    return rec


def verify_table(steps, trials):
    import tree_walk as tw
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    out = []
    for name, parent in (("branching[4,2,1,1]", tw.from_branching([4, 2, 1, 1])), ("irregular64", tw.irregular())):
        tree = TokenTree(parent)
        N = tree.num_nodes
        g = torch.Generator().manual_seed(N)
        tl = (torch.randn(1, N + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(DEV)
        tok = torch.zeros(1, N, dtype=torch.long, device=DEV)
        for s in tree.internal_slots:
            tok[0, torch.tensor(tree.children[s], device=DEV)] = ops.topk_children(tl[:, s], len(tree.children[s]))[0]
        pd = torch.tensor([parent], dtype=torch.int32, device=DEV)
        for kind in ("multinomial", "greedy"):
            spec, noise = ops.ProcSpec(kind, 1.0), PhiloxNoise(seed=1)
            calls = {"verify_tree_distinct": lambda: ops.verify_tree_distinct(tl, tok, tree, spec, noise),
                     "verify_tree_dynamic": lambda: ops.verify_tree_dynamic(tl, tok, pd, spec, noise, tree.depth)}
            us, med = alternate(calls, steps, trials)
            y = us["verify_tree_distinct"]
            out.append(dict(topology=name, nodes=N, processor=kind, trials_us=us, median_us=med,
                            ratio_dynamic_over_distinct=round(med["verify_tree_dynamic"] / med["verify_tree_distinct"], 3),
                            yardstick_spread_max_over_min=round(max(y) / min(y), 3)))
            print(json.dumps(out[-1]), flush=True)
    return out


def loop_table(prompt_len, gen, trials):
    from kv_compact_timing import _llama
    from specdec_amd.sampling import dynamic_tree_speculative_generate, tree_speculative_generate
    from specdec_amd.tree import DynamicTreeSpec, TokenTree
    from specdec_amd.utils.logits_processor import GreedyProcessor
    target, drafter = _llama(16, 0), _llama(4, 1)
    tree = TokenTree.from_branching([4, 2, 1, 1])
    spec = DynamicTreeSpec(4, 4, 4, tree.num_nodes)
    prompt = torch.randint(0, VOCAB, (prompt_len,), generator=torch.Generator().manual_seed(3)).tolist()

    def run(kind, n):
        torch.manual_seed(5)
        trace = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "dynamic":
            toks, rate = dynamic_tree_speculative_generate(prompt, drafter, target, logits_processor=GreedyProcessor(),
                                                           max_gen_len=n, eos_tokens_id=[-1], spec=spec, trace=trace)
        else:
            toks, rate = tree_speculative_generate(prompt, drafter, target, logits_processor=GreedyProcessor(), max_gen_len=n,
                                                   eos_tokens_id=[-1], tree=tree, children="topk", trace=trace)
        torch.cuda.synchronize()
        return toks, trace, time.perf_counter() - t0

    for k in ("static_topk", "dynamic"):
        run(k, 16)
    secs, toks, steps = {"static_topk": [], "dynamic": []}, {}, {}
    for _ in range(trials):
        for k in secs:
            toks[k], tr, s = run(k, gen)
            steps[k] = tr
            secs[k].append(round(s, 4))
    med = {k: statistics.median(v) for k, v in secs.items()}
    res = dict(prompt_tokens=prompt_len, generated=gen, processor="greedy", nodes_per_target_forward=tree.num_nodes,
               static_tree="from_branching([4,2,1,1])", dynamic_spec=repr(spec),
               target="Llama-3.2-1B shape, random init, bf16", drafter="4 layers of the same width, random init, bf16",
               same_tokens=toks["dynamic"] == toks["static_topk"], trials_s=secs, median_s=med,
               tokens_per_s={k: round(len(toks[k]) / med[k], 1) for k in secs},
               accepted_per_target_forward={k: round(sum(st["n"] for st in steps[k]) / max(1, len(steps[k])), 3) for k in secs},
               note="random-init models: the acceptance figures say little about real drafters")
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--gen", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_dynamic_timing.json"))
    args = ap.parse_args()
    res = dict(vocab=VOCAB, dtype="bf16", batch=1, steps=args.steps, trials=args.trials, device=torch.cuda.get_device_name(0),
               grow_level=grow_table(args.steps, args.trials), verify=verify_table(args.steps, args.trials))
    if not args.skip_loop:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        res["loop"] = loop_table(args.prompt, args.gen, args.trials)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
