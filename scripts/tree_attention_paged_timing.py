"""What the page walk costs tree attention, and what a paged call saves a paged user.

    python scripts/tree_attention_paged_timing.py [--steps 100] [--trials 5] [--out FILE]   (GPU)

Shapes of Llama-3-8B (32 / 8 heads, D = 128), rows as scripts/tree_attention_ragged_timing.py builds them.  B = 8 with
the ragged prefixes 512..8192 and a uniform 8 x 2048 batch; R in {29, 65}; page size S in {16, 128}; bf16 and FP8
pools.  Three candidates alternate in one process, device events around each block of steps after a warm-up, the
median of the trials and their spread (microseconds per call, Python wrapper included):

  a. contiguous   sd_tree_attention_ragged(_fp8) on the same data held as [B, Hkv, L, D]: the kernel the page walk is
                  charged against
  b. paged        sd_tree_attention_paged through a shuffled block table
  c. gather       what a paged user does without (b): gather every sequence's pages into a contiguous tensor, then (a)

and, in the same file, sd_kv_store_paged and sd_kv_compact_paged against their contiguous counterparts.
Writes profiles/tree_attention_paged_timing.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from tree_attention_ragged_timing import HKV, SPREAD, inputs, measure  # noqa: E402

F8 = torch.float8_e4m3fn


def paged(seq, S, table):
    """seq [B, H, max_pages * S, D] scattered into a pool [num_pages, H, S, D]: page p of sequence b at table[b, p]."""
    B, H, L, D = seq.shape
    pool = torch.zeros(int(table.max()) + 1, H, S, D, dtype=seq.dtype, device=seq.device)
    pool.view(torch.uint8)[table.flatten().long()] = seq.view(torch.uint8).view(B, H, L // S, S, -1).transpose(1, 2).flatten(0, 1)
    return pool


def gathered(pool, table):
    """The contiguous [B, H, max_pages * S, D] copy of the pages a table names."""
    B, P = table.shape
    pages = pool.view(torch.uint8)[table.long()]                            # [B, max_pages, H, S, bytes]
    return pages.transpose(1, 2).reshape(B, pool.shape[1], P * pool.shape[2], -1).view(pool.dtype)


def summary(us, med):
    return dict(trials_us=us, median_us=med, spread_us={n: [min(t), max(t)] for n, t in us.items()})


def attention_table(steps, trials):
    from specdec_amd import ops
    rows = []
    for tag, prefixes in (("ragged", SPREAD), ("uniform", (2048,) * 8)):
        for R in (29, 65):
            for fp8 in (False, True):
                for S in (16, 128):
                    q, k, v, limit, bits, kv_len, base = inputs(prefixes, R)
                    B, max_pages = len(prefixes), -(-(max(prefixes) + R) // S)
                    pad = max_pages * S - k.shape[2]
                    k, v = (torch.nn.functional.pad(t, (0, 0, 0, pad)) for t in (k, v))
                    scales = {}
                    if fp8:
                        s = torch.full((HKV,), 0.05, device="cuda")
                        k, v, scales = (k.float() / 0.05).to(F8), (v.float() / 0.05).to(F8), dict(k_scale=s, v_scale=s)
                    table = torch.randperm(B * max_pages + 64, device="cuda")[:B * max_pages].view(B, max_pages).int()
                    kp, vp = paged(k, S, table), paged(v, S, table)
                    cap = max(prefixes) + R
                    calls = {
                        "contiguous": lambda: ops.tree_attention(q, k, v, limit, bits, base, kv_len=kv_len, kv_cap=cap, **scales),
                        "paged": lambda: ops.tree_attention(q, kp, vp, limit, bits, base, kv_len=kv_len, kv_cap=cap,
                                                            block_table=table, **scales),
                        "gather": lambda: ops.tree_attention(q, gathered(kp, table), gathered(vp, table), limit, bits, base,
                                                             kv_len=kv_len, kv_cap=cap, **scales),
                    }
                    same = all(torch.equal(calls["contiguous"]().view(torch.int16), calls[n]().view(torch.int16))
                               for n in ("paged", "gather"))
                    us, med = measure(calls, steps, trials)
                    rows.append(dict(batch=tag, B=B, prefixes=list(prefixes), R=R, kv="fp8" if fp8 else "bf16", page_size=S,
                                     bit_identical=same, **summary(us, med),
                                     paged_over_contiguous=round(med["paged"] / med["contiguous"], 3),
                                     gather_over_paged=round(med["gather"] / med["paged"], 2)))
                    print(json.dumps(rows[-1]), flush=True)
                    del k, v, kp, vp
    return rows


def store_compact_table(steps, trials):
    """A layer's store (B = 8 x 2048, R = 65) and the compaction of 32 layers' K and V (R = 29 slots, depth 8)."""
    from specdec_amd import ops
    B, H, D, prefix, rows = 8, HKV, 128, 2048, []
    dev = "cuda"
    pos = torch.full((B,), prefix, dtype=torch.long, device=dev)
    for S in (16, 128):
        max_pages = -(-(prefix + 65) // S)
        L = max_pages * S
        table = torch.randperm(B * max_pages + 64, device=dev)[:B * max_pages].view(B, max_pages).int()
        k_new, v_new = (torch.randn(B, 65, H, D, device=dev, dtype=torch.bfloat16).transpose(1, 2) for _ in range(2))
        s = torch.full((H,), 0.05, device=dev)
        for fp8 in (False, True):
            dt = F8 if fp8 else torch.bfloat16
            flat = [torch.zeros(B, H, L, D, device=dev).to(dt) for _ in range(2)]
            pools = [torch.zeros(B * max_pages + 64, H, S, D, device=dev).to(dt) for _ in range(2)]
            kw = dict(k_scale=s, v_scale=s) if fp8 else {}
            calls = {"paged": lambda: ops.kv_store_paged(k_new, v_new, pools[0], pools[1], table, pos, **kw)}
            if fp8:
                calls["contiguous"] = lambda: ops.kv_store_fp8(k_new, v_new, flat[0], flat[1], s, s, 0, pos_dev=pos)
            else:                                     # no HIP counterpart: two slice copies at a host position
                calls["contiguous"] = lambda: (flat[0][:, :, prefix:prefix + 65].copy_(k_new), flat[1][:, :, prefix:prefix + 65].copy_(v_new))
            us, med = measure(calls, steps, trials)
            rows.append(dict(op="kv_store", page_size=S, kv="fp8" if fp8 else "bf16", R=65, **summary(us, med)))
            print(json.dumps(rows[-1]), flush=True)
        flat = [torch.zeros(B, H, L, D, device=dev, dtype=torch.bfloat16) for _ in range(64)]
        pools = [torch.zeros(B * max_pages + 64, H, S, D, device=dev, dtype=torch.bfloat16) for _ in range(64)]
        path = torch.tensor([[0, 2, 5, 9, 14, 20, 24, 28]] * B, dtype=torch.int32, device=dev)
        count = torch.full((B,), 8, dtype=torch.int32, device=dev)
        calls = {"paged": lambda: ops.kv_compact(pools, path, count, 0, num_slots=29, base_dev=pos, block_table=table),
                 "contiguous": lambda: ops.kv_compact(flat, path, count, 0, num_slots=29, base_dev=pos)}
        us, med = measure(calls, steps, trials)
        rows.append(dict(op="kv_compact", page_size=S, kv="bf16", tensors=64, depth=8, **summary(us, med)))
        print(json.dumps(rows[-1]), flush=True)
        del flat, pools
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_attention_paged_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_attention_paged_timing.py measures on the GPU; none found")
    res = dict(device=torch.cuda.get_device_name(0), model="Llama-3-8B heads (32 / 8, D = 128)", steps=args.steps,
               trials=args.trials, attention=attention_table(args.steps, args.trials),
               store_compact=store_compact_table(args.steps, args.trials))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
