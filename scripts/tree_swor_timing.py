"""Measurements of the without-replacement token trees, written to profiles/tree_swor_timing.json.

 (a) sd_verify_tree_swor against THIS tree's sd_verify_tree (not an older build's) on the same trees, B = 1, V = 128256, bf16 (the SWOR mass launches
     do strictly more per element; the ratio is reported whatever it is);
 (b) sample_distinct at k = 4 against four sample_rows calls and against topk_children.
     Method as scripts/tree_timing.py: HIP events around `steps` back-to-back calls after a warm-up, the median
     of `trials` such runs, microseconds per call.
 --acceptance: the CPU table only (host models, no GPU): accepted drafts per target forward of the three child
     rules (iid, top-c, without replacement) on the FakeLM pair of §4c, at sigma = 1 under T = 1 and under a peaked
     drafter (T = 0.3).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "speculative-decoding_amd")]
VOCAB = 128256
BRANCHINGS = ([4], [2, 2], [4, 2, 1, 1])


def swor_acceptance(target, drafter, parent, steps, seed, proc):
    """tree_walk.simulate_acceptance with the children of a slot drawn without replacement from the exact q and
    walked by tree_swor_ref.walk."""
    import tree_swor_ref as sw
    import tree_walk as tw
    from oracle import specdec_ref as ref
    rng = np.random.default_rng(seed)
    nrows = target.bank.shape[0]
    Pb = ref.process(target.bank.cpu(), proc, exact=True).double().numpy()
    Qb = ref.process(drafter.bank.cpu(), proc, exact=True).double().numpy()
    row = lambda t, p: (int(t) * 31 + p * target.pos_mult) % nrows   # noqa: E731
    N, depths, ch = len(parent), tw.node_depths(parent), sw.children_of(parent)
    prev, cur, total = 3, 8, 0
    for _ in range(steps):
        tok = np.full(N, -1, dtype=np.int64)
        idx = [row(prev, cur - 1)] + [0] * N
        for s in range(N + 1):                         # parents come before their children
            if ch[s]:
                q = Qb[idx[s]] / Qb[idx[s]].sum()
                n = min(len(ch[s]), int((q > 0).sum()))
                tok[ch[s][:n]] = rng.choice(len(q), size=n, replace=False, p=q)
                for c in ch[s]:
                    idx[c + 1] = row(max(int(tok[c]), 0), cur - 1 + depths[c])
        o = sw.walk(Pb[idx], Qb[idx], tok, parent, lambda c, j, frac, slack: not (rng.random() > frac), exact=True)
        total += o.n
        prev = rng.choice(len(o.weights), p=o.weights / o.weights.sum())
        cur += o.n + 1
    return total / steps


def acceptance_table(steps):
    import fakelm
    import tree_distinct_walk as dw
    import tree_walk as tw
    from oracle import specdec_ref as ref
    target, drafter = fakelm.make_pair(4096, sigma=1.0)
    rows = []
    for T in (1.0, 0.3):
        proc = ref.Processor("multinomial", T)
        for widths in BRANCHINGS:
            parent = tw.from_branching(widths)
            rows.append(dict(temperature=T, branching=widths, nodes=len(parent),
                             iid=round(tw.simulate_acceptance(target, drafter, parent, steps, 7, proc), 3),
                             topk=round(dw.simulate_acceptance(target, drafter, parent, steps, 7, proc), 3),
                             distinct=round(swor_acceptance(target, drafter, parent, steps, 7, proc), 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def timed(fn, steps, trials):
    import torch
    for _ in range(10):
        fn()
    out = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return round(statistics.median(out), 2)


def timing_tables(steps, trials):
    import torch
    import tree_walk as tw
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    dev, spec, g = "cuda", ops.ProcSpec("multinomial", 1.0), torch.Generator().manual_seed(3)
    verify = []
    for widths in BRANCHINGS:
        tree = TokenTree(tw.from_branching(widths))
        N, internal = tree.num_nodes, tree.internal_slots
        tl = (torch.randn(1, N + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
        dl = (tl[:, internal].float() + torch.randn(1, len(internal), VOCAB, generator=g).to(dev)).to(torch.bfloat16)
        tok = torch.empty(1, N, dtype=torch.long, device=dev)
        for i, s in enumerate(internal):               # children as the loop draws them
            tok[0, tree.children[s]] = ops.sample_distinct(dl[:, i], len(tree.children[s]), spec, PhiloxNoise(seed=1, offset=s))[0][0]
        us = {name: timed(lambda fn=fn: fn(tl, dl, tok, tree, spec, PhiloxNoise(seed=2, offset=0), want_tokens=False), steps, trials)
              for name, fn in (("verify_tree", ops.verify_tree), ("verify_tree_swor", ops.verify_tree_swor))}
        verify.append(dict(branching=widths, nodes=N, us=us, ratio_swor_over_tree=round(us["verify_tree_swor"] / us["verify_tree"], 3)))
        print(json.dumps(verify[-1]), flush=True)
    rows = (torch.randn(1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
    four = rows.expand(4, VOCAB).contiguous()
    draw = dict(sample_distinct_k4=timed(lambda: ops.sample_distinct(rows, 4, spec, PhiloxNoise(seed=1, offset=0)), steps, trials),
                four_sample_rows_calls=timed(lambda: [ops.sample_rows(rows, spec, PhiloxNoise(seed=1, offset=i)) for i in range(4)], steps, trials),
                one_sample_rows_call_of_4_rows=timed(lambda: ops.sample_rows(four, spec, PhiloxNoise(seed=1, offset=0)), steps, trials),
                topk_children_k4=timed(lambda: ops.topk_children(rows, 4), steps, trials))
    print(json.dumps(draw), flush=True)
    return verify, draw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--acceptance", action="store_true", help="the CPU table only (host models, no GPU)")
    ap.add_argument("--accept-steps", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_swor_timing.json"))
    args = ap.parse_args()
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res.setdefault("commands", {})["acceptance" if args.acceptance else "timing"] = " ".join(sys.argv)
    if args.acceptance:
        res["acceptance"] = dict(vocab=4096, sigma=1.0, steps=args.accept_steps, rows=acceptance_table(args.accept_steps))
    else:
        verify, draw = timing_tables(args.steps, args.trials)
        res["timing"] = dict(vocab=VOCAB, dtype="bf16", batch=1, steps=args.steps, trials=args.trials, unit="us per call",
                             verify=verify, draw=draw)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
