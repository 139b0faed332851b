"""What reading the lengths on the device costs tree attention, and what one ragged call buys.

    python scripts/tree_attention_ragged_timing.py [--steps 100] [--trials 5] [--out FILE]   (GPU)

Shapes of Llama-3-8B (32 / 8 heads, D = 128), bf16, rows as scripts/tree_attention_timing.py builds them (one
catch-up row, then tree nodes under a causal window).  The candidates of a shape alternate in one process,
device events around each block of steps after a warm-up, the median of the trials (microseconds per
call, Python wrapper included).

1. uniform: B in {1, 8}, prefix in {512, 2048, 8192}, R in {29, 65}, every sequence prefix + R long.
   sd_tree_attention (host kv_len: proportional splits) against sd_tree_attention_ragged (device lengths,
   kv_cap = prefix + R: fixed chunks), with the split count and the chunk rule each ran with.
2. ragged: B = 8 with prefixes spread over 512..8192.  One sd_tree_attention_ragged call against the
   only expression without it: eight batch-1 sd_tree_attention calls, each with its own host kv_len.

Writes profiles/tree_attention_ragged_timing.json.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HQ, HKV, D = 32, 8, 128
SPREAD = (512, 1024, 2048, 3072, 4096, 5120, 6144, 8192)


def chunk_rule(B, L):
    """(chunk_tiles, C) of the auto rule (ta_chunk_tiles of csrc/tree_attention.hip, checked against the library's C)."""
    from specdec_amd import ops
    tiles, slots = (L + 63) // 64, -(-256 // (B * HKV))
    ct = min(tiles, max(4, -(-tiles // slots), -(-tiles // 64)))
    C = ops.tree_attention_chunks(B, HKV, L, 0)
    assert C == -(-tiles // ct) == ops.tree_attention_chunks(B, HKV, L, ct), (B, L, ct, C)
    return ct, C


def inputs(prefixes, R):
    """q, k, v, kv_limit, win_bits and per-sequence (kv_len, win_base) for sequences of prefix + R positions."""
    dev, B, L = "cuda", len(prefixes), max(prefixes) + R
    torch.manual_seed(0)
    q = torch.randn(B, HQ, R, D, device=dev, dtype=torch.bfloat16)
    k, v = (torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
    pre = torch.tensor(prefixes, device=dev)
    limit = (pre[:, None] + 1).expand(B, R).int().contiguous()            # row 0 sees itself; cur = prefix + 1
    words = [0] + [(1 << (i + 1)) - 1 for i in range(R - 1)]
    bits = torch.tensor([[w - (1 << 64) if w >> 63 else w for w in words]] * B, device=dev)
    return q, k, v, limit, bits, pre + R, pre + 1


def measure(calls, steps, trials):
    from tree_attention_timing import timed
    for _ in range(10):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(trials):
        for name, fn in calls.items():
            us[name].append(round(timed(fn, steps), 2))
    return us, {name: statistics.median(t) for name, t in us.items()}


def uniform_table(steps, trials):
    from specdec_amd import ops
    rows = []
    for B in (1, 8):
        for prefix in (512, 2048, 8192):
            for R in (29, 65):
                q, k, v, limit, bits, kv_len, base = inputs((prefix,) * B, R)
                L = prefix + R
                calls = {"sd_tree_attention": lambda: ops.tree_attention(q, k, v, limit, bits, prefix + 1),
                         "sd_tree_attention_ragged": lambda: ops.tree_attention(q, k, v, limit, bits, base, kv_len=kv_len)}
                diff = float((calls["sd_tree_attention"]().float() - calls["sd_tree_attention_ragged"]().float()).abs().max())
                us, med = measure(calls, steps, trials)
                ct, C = chunk_rule(B, L)
                rows.append(dict(B=B, prefix=prefix, R=R, splits=ops.tree_attention_splits(B, HKV, L), chunk_tiles=ct,
                                 chunks=C, max_abs_diff=diff, trials_us=us, median_us=med,
                                 ragged_over_uniform=round(med["sd_tree_attention_ragged"] / med["sd_tree_attention"], 3)))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def ragged_table(steps, trials):
    from specdec_amd import ops
    rows = []
    for R in (29, 65):
        q, k, v, limit, bits, kv_len, base = inputs(SPREAD, R)
        B, L = len(SPREAD), max(SPREAD) + R
        one = [(q[b:b + 1], k[b:b + 1], v[b:b + 1], limit[b:b + 1].contiguous(), bits[b:b + 1].contiguous(), SPREAD[b] + 1,
                SPREAD[b] + R) for b in range(B)]

        def ragged():
            return ops.tree_attention(q, k, v, limit, bits, base, kv_len=kv_len)

        def per_sequence():
            return [ops.tree_attention(qb, kb, vb, lb, wb, wbase, kv_len=n) for qb, kb, vb, lb, wb, wbase, n in one]

        diff = float((ragged().float() - torch.cat(per_sequence()).float()).abs().max())
        us, med = measure({"one_ragged_call": ragged, "batch1_calls": per_sequence}, steps, trials)
        ct, C = chunk_rule(B, L)
        rows.append(dict(B=B, prefixes=list(SPREAD), R=R, chunk_tiles=ct, chunks=C, max_abs_diff=diff, trials_us=us,
                         median_us=med, batch1_over_ragged=round(med["batch1_calls"] / med["one_ragged_call"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_attention_ragged_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_attention_ragged_timing.py measures on the GPU; none found")
    res = dict(device=torch.cuda.get_device_name(0), model="Llama-3-8B heads (32 / 8, D = 128)", dtype="bf16",
               steps=args.steps, trials=args.trials, uniform=uniform_table(args.steps, args.trials),
               ragged=ragged_table(args.steps, args.trials))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
