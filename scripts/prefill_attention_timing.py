"""What sd_prefill_attention costs next to what a user can do without it.

    python scripts/prefill_attention_timing.py [--steps 20] [--trials 5] [--out FILE]   (GPU)

Llama-3-8B heads (32 / 8, D = 128), one layer's attention.  Pure prefill of 2048 and 8192 rows at B = 1, and a 512-row
chunk behind a 7680-key prefix at B = 1 and B = 8; over a contiguous bf16 cache and over FP8 pools behind a shuffled
block table (S = 16).  The candidates of a case alternate in one process, device events around each block of steps
after a warm-up, the median of the trials with the lowest and highest (microseconds per call, Python wrapper included):

  kernel   ops.prefill_attention (one launch)
  sdpa     F.scaled_dot_product_attention(is_causal=True, enable_gqa=True): pure prefill on the contiguous bf16 cache only
  gather   what the other cases leave a torch user: (gather the pages, dequantise,) sdpa with a boolean mask built once
  chain    the 128-row ops.tree_attention calls that cover the same rows today, descriptors built once outside the timing

The operations (4 Hq D per visible (row, key) pair) and the K/V bytes a perfect kernel reads once are computed from the
shapes; mfma_share and hbm_share are those over the kernel's time, against 2.5 PFLOP/s (the public dense bf16 figure of
the MI355X) and 8 TB/s.  Writes profiles/prefill_attention_timing.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from tree_attention_paged_timing import gathered, paged, summary  # noqa: E402
from tree_attention_ragged_timing import measure  # noqa: E402

HQ, HKV, D, S, F8 = 32, 8, 128, 16, torch.float8_e4m3fn
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8e12
CASES = [(1, 0, 2048), (1, 0, 8192), (1, 7680, 512), (8, 7680, 512)]       # (B, prefix, rows)


def chain(q, k, v, prefix, R, **kw):
    """The tree-attention calls that cover rows [0, R) 128 at a time: causal kv_limit, no window bits."""
    from specdec_amd import ops
    B = q.shape[0]
    parts = []
    for r0 in range(0, R, 128):
        n = min(128, R - r0)
        limit = (prefix + r0 + 1 + torch.arange(n, device="cuda")).int().expand(B, n).contiguous()
        bits = torch.zeros(B, n, dtype=torch.long, device="cuda")
        kv_len = torch.full((B,), prefix + r0 + n, dtype=torch.long, device="cuda")
        parts.append((q[:, :, r0:r0 + n], limit, bits, kv_len))
    return lambda: [ops.tree_attention(qq, k, v, limit, bits, 0, kv_len=kv_len, kv_cap=prefix + R, **kw)
                    for qq, limit, bits, kv_len in parts]


def table(steps, trials):
    from specdec_amd import ops
    rows, dev = [], "cuda"
    for B, prefix, R in CASES:
        L = prefix + R
        torch.manual_seed(0)
        q = torch.randn(B, HQ, R, D, device=dev, dtype=torch.bfloat16)
        k, v = (torch.randn(B, HKV, L, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
        mask = torch.arange(L, device=dev)[None, :] <= prefix + torch.arange(R, device=dev)[:, None]
        pairs = B * (R * prefix + R * (R + 1) // 2)
        for kind in ("bf16 contiguous", "fp8 paged S=16"):
            if kind.startswith("bf16"):
                calls = {"kernel": lambda: ops.prefill_attention(q, k, v, L),
                         "gather": lambda: F.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True),
                         "chain": chain(q, k, v, prefix, R)}
                if prefix == 0:
                    calls["sdpa"] = lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
                kv_bytes = 2 * B * HKV * L * D * 2
            else:
                s = torch.full((HKV,), 0.05, device=dev)
                tab = torch.randperm(B * (L // S) + 64, device=dev)[:B * (L // S)].view(B, L // S).int()
                kp, vp = (paged((t.float() / 0.05).to(F8), S, tab) for t in (k, v))
                deq = lambda pool: (gathered(pool, tab).float() * 0.05).to(torch.bfloat16)
                calls = {"kernel": lambda: ops.prefill_attention(q, kp, vp, L, block_table=tab, k_scale=s, v_scale=s),
                         "gather": lambda: F.scaled_dot_product_attention(q, deq(kp), deq(vp), attn_mask=mask, enable_gqa=True),
                         "chain": chain(q, kp, vp, prefix, R, block_table=tab, k_scale=s, v_scale=s)}
                kv_bytes = 2 * B * HKV * L * D
            ref = calls["gather"]().transpose(1, 2).float()
            diff = float((calls["kernel"]().float() - ref).abs().max())
            us, med = measure(calls, steps, trials)
            least = max(4 * HQ * D * pairs / PEAK_FLOPS, kv_bytes / PEAK_BYTES) * 1e6
            rows.append(dict(B=B, prefix=prefix, rows=R, cache=kind, max_abs_diff_vs_gather=diff, **summary(us, med),
                             workgroups=B * HKV * -(-R // 32), flops=4 * HQ * D * pairs, kv_bytes=kv_bytes,
                             mfma_share=round(4 * HQ * D * pairs / PEAK_FLOPS * 1e6 / med["kernel"], 4),
                             hbm_share=round(kv_bytes / PEAK_BYTES * 1e6 / med["kernel"], 4),
                             bound="mfma" if 4 * HQ * D * pairs / PEAK_FLOPS > kv_bytes / PEAK_BYTES else "hbm",
                             least_us=round(least, 2),
                             **{f"{n}_over_kernel": round(med[n] / med["kernel"], 2) for n in med if n != "kernel"}))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_attention_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefill_attention_timing.py measures on the GPU; none found")
    res = dict(device=torch.cuda.get_device_name(0), model="Llama-3-8B heads (32 / 8, D = 128)", steps=args.steps,
               trials=args.trials, peaks=dict(flops=PEAK_FLOPS, bytes_per_s=PEAK_BYTES), attention=table(args.steps, args.trials))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
