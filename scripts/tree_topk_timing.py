"""What the distinct-children tree verify costs next to the iid one, and what top-k children buy.

    python scripts/tree_topk_timing.py [--steps 300] [--trials 5] [--out FILE]                  (GPU)
    python scripts/tree_topk_timing.py --acceptance [--accept-steps 3000] [--out FILE]          (CPU only)

1. One sd_verify_tree_distinct against one sd_verify_tree (the yardstick: its code is the parent
   commit's) at B = 1, V = 128256, bf16, on the topologies of DESIGN.md §4e's table — [2,1], [4,1],
   [3,2,1], [4,2,1,1] and chains(K, 4), K in {1, 2, 4, 8} — under multinomial and under greedy.  The two
   calls alternate block by block in one process, device events around each block of steps after a
   warm-up, the median of the trials (microseconds per call).
2. --acceptance: accepted drafts per target forward on the FakeLM pair of DESIGN.md §4c / §4e (vocab
   4096, sigma = 1) for children="topk" against iid children on the same trees, under multinomial and
   under greedy, by the host models (tests/tree_distinct_walk.py, tests/tree_ref.py); no GPU.

Both write into the same JSON file (each run updates its own key).  For kernel times:
`rocprofv3 --kernel-trace --stats -- python scripts/tree_topk_timing.py --trials 1` (no counters in
the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

GAMMA, VOCAB = 4, 128256
BRANCHINGS = ([2, 1], [4, 1], [3, 2, 1], [4, 2, 1, 1])
CHAINS = (1, 2, 4, 8)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def _topologies(TokenTree):
    out = [(f"branching{b}".replace(" ", ""), TokenTree.from_branching(b)) for b in BRANCHINGS]
    return out + [(f"chains({K},{GAMMA})", TokenTree.chains(K, GAMMA)) for K in CHAINS]


def verify_table(steps, trials):
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    dev = "cuda"
    rows = []
    for name, tree in _topologies(TokenTree):
        N, internal = tree.num_nodes, tree.internal_slots
        g = torch.Generator().manual_seed(N)
        tl = (torch.randn(1, N + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
        dl = (tl[:, internal].float() + torch.randn(1, len(internal), VOCAB, generator=g).to(dev)).to(torch.bfloat16)
        # the drafter's top-c tokens by slot (distinct children); the iid call takes the same ids
        tok = torch.zeros(1, N, dtype=torch.long, device=dev)
        for i, s in enumerate(internal):
            best = ops.topk_children(dl[:, i], len(tree.children[s]))[0]
            tok[0, torch.tensor(tree.children[s], device=dev)] = best
        for kind in ("multinomial", "greedy"):
            spec, noise = ops.ProcSpec(kind, 1.0), PhiloxNoise(seed=1)
            calls = {
                "verify_tree_distinct": lambda: ops.verify_tree_distinct(tl, tok, tree, spec, noise),
                "verify_tree": lambda: ops.verify_tree(tl, dl, tok, tree, spec, noise),
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
                topology=name, nodes=N, processor=kind, trials_us=us, median_us=med,
                rows_read=dict(verify_tree_distinct=N + 1, verify_tree=N + 1 + len(internal)),
                full_vocab_launches_after_stats=dict(verify_tree_distinct=1, verify_tree=tree.max_children + 1),
                ratio_distinct_over_tree=round(med["verify_tree_distinct"] / med["verify_tree"], 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def _iid_acceptance(target, drafter, parent, steps, seed, greedy):
    """tree_walk.simulate_acceptance, and its greedy form: every child of a slot is the drafter's
    argmax (what sample_rows returns under GreedyProcessor), tested by sd_verify_tree's rule on the
    softmax rows, the emitted token the argmax of the final weights."""
    import tree_ref as tref
    import tree_walk as tw
    from oracle import specdec_ref as ref
    if not greedy:
        return tw.simulate_acceptance(target, drafter, parent, steps, seed)
    proc = tw.PROCS["greedy"]
    rng = np.random.default_rng(seed)
    nrows = target.bank.shape[0]
    Pb = ref.process(target.bank.cpu(), proc, exact=True).double().numpy()
    Qb = ref.process(drafter.bank.cpu(), proc, exact=True).double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % nrows   # noqa: E731
    N, depths = len(parent), tw.node_depths(parent)
    prev, cur, total = 3, 8, 0
    for _ in range(steps):
        tok = np.zeros(N, dtype=np.int64)
        idx = [row(prev, cur - 1)] + [0] * N
        for i in range(N):
            tok[i] = int(np.argmax(Qb[idx[parent[i] + 1]]))
            idx[i + 1] = row(tok[i], cur - 1 + depths[i])
        o = tref.walk(Pb[idx], Qb[idx], tok, parent, lambda c, j, frac, slack: not (rng.random() > frac))
        total += o.n
        prev = int(np.argmax(o.weights))
        cur += o.n + 1
    return total / steps


def acceptance_table(steps):
    import fakelm
    import tree_distinct_walk as dw
    import tree_walk as tw
    target, drafter = fakelm.make_pair(4096, sigma=1.0)
    trees = [(str(b).replace(" ", ""), tw.from_branching(b)) for b in BRANCHINGS]
    trees += [(f"chains({K},{GAMMA})", tw.chains(K, GAMMA)) for K in CHAINS]
    rows = []
    for name, parent in trees:
        rec = dict(topology=name, nodes=len(parent))
        for kind, greedy in (("multinomial", False), ("greedy", True)):
            rec[f"{kind}_topk"] = round(dw.simulate_acceptance(target, drafter, parent, steps, 7, greedy=greedy), 3)
            rec[f"{kind}_iid"] = round(_iid_acceptance(target, drafter, parent, steps, 7, greedy), 3)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--acceptance", action="store_true", help="the CPU table only (host models, no GPU)")
    ap.add_argument("--accept-steps", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_topk_timing.json"))
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.acceptance:
        res["acceptance"] = dict(vocab=4096, sigma=1.0, steps=args.accept_steps, unit="accepted drafts per target forward",
                                 rows=acceptance_table(args.accept_steps))
    else:
        res["verify"] = dict(vocab=VOCAB, dtype="bf16", batch=1, steps=args.steps, trials=args.trials,
                             yardstick="verify_tree (unchanged from the parent commit)",
                             device=torch.cuda.get_device_name(0), rows=verify_table(args.steps, args.trials))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
