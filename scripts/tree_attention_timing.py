"""What tree attention costs next to the torch expression, and what it buys the cached tree loop.

    python scripts/tree_attention_timing.py [--steps 100] [--trials 5] [--gen 128] [--prompts 512 1536] [--out FILE]   (GPU)

1. ops.tree_attention (sd_tree_attention) against F.scaled_dot_product_attention with the dense additive
   mask [B, 1, R, L] and K/V repeated across the query heads of a group, which is what transformers'
   sdpa attention does when it is handed a mask.  Shapes of Llama-3-8B (32 / 8 heads, D = 128) and
   Llama-3.2-1B (32 / 8 heads, D = 64), bf16; R in {29, 65} rows (one catch-up row, then tree nodes under a
   causal window), prefix in {512, 2048, 8192}, B in {1, 8}.  The two alternate in one process, device
   events around each block of steps after a warm-up, the median of the trials (microseconds per call).
   Recorded besides: the split count the shapes chose and the K/V bytes (2 * B * Hkv * kv_len * D * 2)
   over the kernel's time as a fraction of the 8 TB/s HBM peak.  The time is the whole call's, Python
   wrapper included, so the fraction is a lower bound on the kernels' own.
2. tree_speculative_generate(use_cache=True) with attention="mask" and attention="kernel", DynamicCache
   and StaticCache, on scripts/kv_compact_timing.py's models and settings; tokens per second.

Writes profiles/tree_attention_timing.json.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_PEAK = 8.0e12
MODELS = {"Llama-3-8B": (32, 8, 128), "Llama-3.2-1B": (32, 8, 64)}


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
    dev, rows = "cuda", []
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            for prefix in (512, 2048, 8192):
                for R in (29, 65):
                    g = torch.Generator().manual_seed(0)
                    L = prefix + R
                    q = torch.randn(B, Hq, R, D, generator=g).to(torch.bfloat16).to(dev)
                    k, v = (torch.randn(B, Hkv, L, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
                    nodes = R - 1                                       # row 0 is a catch-up token, then the nodes
                    limit = torch.full((B, R), prefix + 1, dtype=torch.int32, device=dev)   # row 0 sees itself; cur = prefix + 1
                    words = [0] + [(1 << (i + 1)) - 1 for i in range(nodes)]
                    bits = torch.tensor([[w - (1 << 64) if w >> 63 else w for w in words]] * B, device=dev)
                    j = torch.arange(L, device=dev)
                    rel = (j - (prefix + 1)).clamp(0, 63)
                    allow = (j < limit[:, :, None]) | ((((bits[:, :, None] >> rel) & 1) == 1) & (j > prefix))
                    mask = torch.zeros(B, 1, R, L, dtype=torch.bfloat16, device=dev)
                    mask.masked_fill_(~allow[:, None], torch.finfo(torch.bfloat16).min)

                    def kernel():
                        return ops.tree_attention(q, k, v, limit, bits, prefix + 1)

                    def sdpa():
                        kr, vr = (t.repeat_interleave(Hq // Hkv, 1) for t in (k, v))
                        return F.scaled_dot_product_attention(q, kr, vr, attn_mask=mask).transpose(1, 2)

                    diff = float((kernel().float() - sdpa().float()).abs().max())
                    calls = {"sd_tree_attention": kernel, "sdpa_dense_mask": sdpa}
                    for _ in range(10):
                        for fn in calls.values():
                            fn()
                    torch.cuda.synchronize()
                    us = {name: [] for name in calls}
                    for _ in range(trials):
                        for name, fn in calls.items():
                            us[name].append(round(timed(fn, steps), 2))
                    med = {name: statistics.median(t) for name, t in us.items()}
                    kv_bytes = 2 * B * Hkv * L * D * 2
                    rows.append(dict(model=model, B=B, prefix=prefix, R=R, splits=ops.tree_attention_splits(B, Hkv, L),
                                     max_abs_diff_to_sdpa=diff, trials_us=us, median_us=med, kv_bytes=kv_bytes,
                                     hbm_fraction=round(kv_bytes / (med["sd_tree_attention"] * 1e-6) / HBM_PEAK, 4),
                                     ratio_sdpa_over_kernel=round(med["sdpa_dense_mask"] / med["sd_tree_attention"], 2)))
                    print(json.dumps(rows[-1]), flush=True)
    return rows


def loop_table(target, drafter, prompt_len, gen, trials):
    from specdec_amd import tree_attention
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.tree import TokenTree
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    tree = TokenTree.from_branching([4, 2, 1, 1])
    prompt = torch.randint(0, 128256, (prompt_len,), generator=torch.Generator().manual_seed(3)).tolist()
    modes = {f"{cache}_{att}": dict(use_cache=True, static_cache=cache == "static", attention=att)
             for cache in ("dynamic", "static") for att in ("mask", "kernel")}

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
    calls = dict(tree_attention.counts)
    for _ in range(trials):
        for k, kw in modes.items():
            toks[k], rates[k], s = run(kw, gen)
            secs[k].append(round(s, 4))
    med = {k: statistics.median(v) for k, v in secs.items()}
    res = dict(prompt_tokens=prompt_len, generated=gen, tree="from_branching([4,2,1,1])", processor="multinomial T=1",
               target="Llama-3.2-1B shape, random init, bf16", drafter="4 layers of the same width, random init, bf16",
               acceptance_rate=rates, trials_s=secs, median_s=med,
               kernel_attention_calls=tree_attention.counts["kernel"] - calls["kernel"],
               tokens_per_s={k: round(len(toks[k]) / med[k], 1) for k in modes},
               kernel_over_mask={c: round(med[f"{c}_mask"] / med[f"{c}_kernel"], 3) for c in ("dynamic", "static")})
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--loop-trials", type=int, default=3)
    ap.add_argument("--prompts", type=int, nargs="+", default=[512, 1536], help="prompt lengths of the loop runs")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_attention_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_attention_timing.py measures on the GPU; none found")
    res = {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["kernel"] = dict(device=torch.cuda.get_device_name(0), dtype="bf16", steps=args.steps, trials=args.trials,
                         hbm_peak_bytes_per_s=HBM_PEAK, rows=kernel_table(args.steps, args.trials))
    save()
    if not args.skip_loop:
        from kv_compact_timing import _llama
        target, drafter = _llama(16, 1), _llama(4, 2)
        res["loop"] = []
        for prompt_len in args.prompts:
            res["loop"].append(loop_table(target, drafter, prompt_len, args.gen, args.loop_trials))
            save()


if __name__ == "__main__":
    main()
