"""What the KV-cache compaction costs, and what the cached tree loop buys.

    python scripts/kv_compact_timing.py [--steps 200] [--trials 5] [--gen 128] [--prompts 512 1536] [--out FILE]   (GPU)

1. One sd_kv_compact launch over a Llama-3-8B cache (64 K/V tensors [1, 8, 2048, 128], bf16) against
   the torch expression of the same move — per tensor one index_select and one index_copy_ (128 launches),
   the accepted length n already on the host, which the kernel does not need.  n in {1, 4, 8, 32}; paths
   from from_branching([4, 2, 1, 1]) (the path to the last leaf) and from chains(1, 32) fed one position
   late (every entry moves down by one: the in-place case).  The two alternate in one process, device
   events around each block of steps after a warm-up, the median of the trials (microseconds per call).
2. tree_speculative_generate at a 512-token prompt (and at the other --prompts) on a random-init Llama-3.2-1B-shaped target (16
   layers, hidden 2048, 8 KV heads, vocab 128256, bf16) with a 4-layer drafter of the same width:
   use_cache=False, use_cache=True and use_cache=True + static_cache=True under one seed (the same
   tokens), alternating, wall clock around a run that ends in a device synchronise; tokens per second.

Writes profiles/kv_compact_timing.json.  For kernel times: `rocprofv3 --kernel-trace --stats -- python
scripts/kv_compact_timing.py --trials 1 --skip-loop` (no counters in the same run).
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

LAYERS, HEADS, LENGTH, HEAD_DIM, BASE = 32, 8, 2048, 128, 1024


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def kernel_table(steps, trials):
    from specdec_amd import ops
    from specdec_amd.tree import TokenTree
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    tensors = [torch.randn(1, HEADS, LENGTH, HEAD_DIM, generator=g).to(torch.bfloat16).to(dev) for _ in range(2 * LAYERS)]
    wide, chain = TokenTree.from_branching([4, 2, 1, 1]), TokenTree.chains(1, 32)
    cases = [("from_branching([4,2,1,1])", wide.path_to(wide.num_nodes - 1), None, wide.num_nodes, n) for n in (1, 4)]
    cases += [("chains(1,32)+1", chain.path_to(31), [i + 1 for i in range(32)], 33, n) for n in (1, 4, 8, 32)]
    rows = []
    for name, full, node_slot, num_slots, n in cases:
        nodes = full[:n]
        slots = [node_slot[i] if node_slot else i for i in nodes]
        path = torch.full((1, len(full)), -1, dtype=torch.int32)
        path[0, :n] = torch.tensor(nodes, dtype=torch.int32)
        path, count = path.to(dev), torch.tensor([n], dtype=torch.int32, device=dev)
        src = torch.tensor([BASE + s for s in slots], device=dev)
        dst = torch.arange(BASE, BASE + n, device=dev)

        def kernel():
            ops.kv_compact(tensors, path, count, BASE, num_slots=num_slots, node_slot=node_slot)

        def torch_ops():
            for t in tensors:
                t.index_copy_(2, dst, t.index_select(2, src))

        # the two compute the same cache (checked once on copies, then timed in place)
        a, b = [t.clone() for t in tensors[:2]], [t.clone() for t in tensors[:2]]
        ops.kv_compact(a, path, count, BASE, num_slots=num_slots, node_slot=node_slot)
        for t in b:
            t.index_copy_(2, dst, t.index_select(2, src))
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        calls = {"sd_kv_compact": kernel, "torch_index_select_copy": torch_ops}
        for _ in range(10):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(trials):
            for k, fn in calls.items():
                us[k].append(round(timed(fn, steps), 2))
        med = {k: statistics.median(v) for k, v in us.items()}
        moved = sum(s != d for d, s in enumerate(slots))
        rows.append(dict(tree=name, n=n, rows_moved_per_head=moved, bytes_moved=moved * 2 * LAYERS * HEADS * HEAD_DIM * 2,
                         equal_to_torch=same, launches=dict(sd_kv_compact=1, torch_index_select_copy=4 * LAYERS),
                         trials_us=us, median_us=med,
                         ratio_torch_over_kernel=round(med["torch_index_select_copy"] / med["sd_kv_compact"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def _llama(layers, seed):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=layers,
                      num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=2048, rope_theta=500000.0,
                      tie_word_embeddings=True)
    torch.manual_seed(seed)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(old)
    return model.eval()


def loop_table(target, drafter, prompt_len, gen, trials):
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.tree import TokenTree
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    tree = TokenTree.from_branching([4, 2, 1, 1])
    prompt = torch.randint(0, 128256, (prompt_len,), generator=torch.Generator().manual_seed(3)).tolist()
    modes = {"uncached": dict(use_cache=False), "cached_dynamic": dict(use_cache=True),
             "cached_static": dict(use_cache=True, static_cache=True)}

    def run(kw, n):
        torch.manual_seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks, rate = tree_speculative_generate(prompt, drafter, target, logits_processor=MultinomialProcessor(1.0),
                                               max_gen_len=n, eos_tokens_id=[-1], tree=tree, **kw)
        torch.cuda.synchronize()
        return toks, rate, time.perf_counter() - t0

    for kw in modes.values():                      # warm-up: every shape of the timed runs' first steps
        run(kw, 24)
    secs, toks, rates = {k: [] for k in modes}, {}, {}
    for _ in range(trials):
        for k, kw in modes.items():
            toks[k], rates[k], s = run(kw, gen)
            secs[k].append(round(s, 4))
    med = {k: statistics.median(v) for k, v in secs.items()}
    res = dict(prompt_tokens=prompt_len, generated=gen, tree="from_branching([4,2,1,1])", processor="multinomial T=1",
               target="Llama-3.2-1B shape, random init, bf16", drafter="4 layers of the same width, random init, bf16",
               acceptance_rate=rates, same_tokens={k: toks[k] == toks["uncached"] for k in modes},
               trials_s=secs, median_s=med, tokens_per_s={k: round(len(toks[k]) / med[k], 1) for k in modes},
               speedup_over_uncached={k: round(med["uncached"] / med[k], 2) for k in modes})
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--loop-trials", type=int, default=3)
    ap.add_argument("--prompts", type=int, nargs="+", default=[512, 1536], help="prompt lengths of the loop runs")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_compact_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_compact_timing.py measures on the GPU; none found")
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["kernel"] = dict(device=torch.cuda.get_device_name(0), tensors=2 * LAYERS, shape=[1, HEADS, LENGTH, HEAD_DIM],
                         dtype="bf16", base=BASE, steps=args.steps, trials=args.trials,
                         rows=kernel_table(args.steps, args.trials))
    save()
    if not args.skip_loop:
        target, drafter = _llama(16, 1), _llama(4, 2)
        res["loop"] = []
        for prompt_len in args.prompts:
            res["loop"].append(loop_table(target, drafter, prompt_len, args.gen, args.loop_trials))
            save()


if __name__ == "__main__":
    main()
