"""What the token-tree verify costs and what a tree buys.

    python scripts/tree_timing.py [--steps 300] [--trials 5] [--out FILE]                  (GPU)
    python scripts/tree_timing.py --acceptance [--accept-steps 3000] [--out FILE]          (CPU only)

1. One sd_verify_tree at B = 1, V = 128256, bf16 on chains(K, 4), K in {1, 2, 4, 8}, and on a
   from_branching tree within the same node budget (4, 8, 16, 32 nodes), against sd_verify_multi(K, 4)
   on the same node count: the three calls alternate in one process, device events around each block
   of steps after a warm-up, the median of the trials (microseconds per call).
2. --acceptance: accepted drafts per target forward of those trees on the FakeLM pair of DESIGN.md
   §4c (vocab 4096, sigma = 1, multinomial), by the host model (tests/tree_walk.simulate_acceptance);
   no GPU.

Both write into the same JSON file (each run updates its own key).  For kernel times:
`rocprofv3 --kernel-trace --stats -- python scripts/tree_timing.py --trials 1` (no counters in the
same run).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

GAMMA, VOCAB = 4, 128256
# node budget 4K -> a tree wide near the root and narrow below, within the budget
BRANCHING = {1: [2, 1], 2: [4, 1], 4: [3, 2, 1], 8: [4, 2, 1, 1]}


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def _tree_inputs(tree, gen, dev):
    N = tree.num_nodes
    tl = (torch.randn(1, N + 1, VOCAB, generator=gen) * 3).to(torch.bfloat16).to(dev)
    internal = tree.internal_slots
    dl = (tl[:, internal].float() + torch.randn(1, len(internal), VOCAB, generator=gen).to(dev)).to(torch.bfloat16)
    tok = torch.randint(0, VOCAB, (1, N), generator=gen).to(dev)
    return tl, dl, tok


def verify_table(steps, trials):
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    dev, spec = "cuda", ops.ProcSpec("multinomial", 1.0)
    rows = []
    for K in (1, 2, 4, 8):
        g = torch.Generator().manual_seed(K)
        mtl = (torch.randn(1, K, GAMMA + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
        mdl = (mtl[:, :, :GAMMA].float() + torch.randn(1, K, GAMMA, VOCAB, generator=g).to(dev)).to(torch.bfloat16)
        mtok = torch.randint(0, VOCAB, (1, K, GAMMA), generator=g).to(dev)
        chain, wide = TokenTree.chains(K, GAMMA), TokenTree.from_branching(BRANCHING[K])
        ctl, cdl, ctok = _tree_inputs(chain, g, dev)
        wtl, wdl, wtok = _tree_inputs(wide, g, dev)
        noise = PhiloxNoise(seed=1)
        calls = {
            "verify_multi": lambda: ops.verify_multi(mtl, mdl, mtok, spec, noise),
            "verify_tree_chains": lambda: ops.verify_tree(ctl, cdl, ctok, chain, spec, noise),
            "verify_tree_branching": lambda: ops.verify_tree(wtl, wdl, wtok, wide, spec, noise),
        }
        for _ in range(20):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(trials):
            for k, fn in calls.items():
                us[k].append(round(timed(fn, steps), 2))
        med = {k: statistics.median(v) for k, v in us.items()}
        rows.append(dict(
            K=K, nodes=K * GAMMA, branching=BRANCHING[K], branching_nodes=wide.num_nodes, trials_us=us, median_us=med,
            rows_read=dict(verify_multi=K * (2 * GAMMA + 1), verify_tree_chains=chain.num_nodes + 1 + len(chain.internal_slots),
                           verify_tree_branching=wide.num_nodes + 1 + len(wide.internal_slots)),
            mass_launches=dict(verify_multi=K + 1, verify_tree_chains=chain.max_children + 1,
                               verify_tree_branching=wide.max_children + 1),
            ratio_chains_over_multi=round(med["verify_tree_chains"] / med["verify_multi"], 3),
            ratio_branching_over_multi=round(med["verify_tree_branching"] / med["verify_multi"], 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def acceptance_table(steps):
    import fakelm
    import tree_walk as tw
    target, drafter = fakelm.make_pair(4096, sigma=1.0)
    rows = []
    for K in (1, 2, 4, 8):
        wide = tw.from_branching(BRANCHING[K])
        rows.append(dict(K=K, nodes=K * GAMMA, branching=BRANCHING[K], branching_nodes=len(wide),
                         accepted_per_forward_chains=round(tw.simulate_acceptance(target, drafter, tw.chains(K, GAMMA), steps, 7), 3),
                         accepted_per_forward_branching=round(tw.simulate_acceptance(target, drafter, wide, steps, 7), 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--acceptance", action="store_true", help="the CPU table only (host model, no GPU)")
    ap.add_argument("--accept-steps", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_timing.json"))
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.acceptance:
        res["acceptance"] = dict(vocab=4096, sigma=1.0, processor="multinomial", steps=args.accept_steps,
                                 rows=acceptance_table(args.accept_steps))
    else:
        res["verify"] = dict(vocab=VOCAB, dtype="bf16", batch=1, gamma=GAMMA, steps=args.steps, trials=args.trials,
                             device=torch.cuda.get_device_name(0), rows=verify_table(args.steps, args.trials))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
