"""What tree attention over an FP8 KV cache costs next to the 16-bit kernel, and the quantising store next to torch.

    python scripts/tree_attention_fp8_timing.py [--steps 100] [--trials 5] [--out FILE]   (GPU)

1. ops.tree_attention with float8_e4m3fn K/V and per-head scales (sd_tree_attention_fp8) against the same call
   with bf16 K/V (sd_tree_attention), on scripts/tree_attention_timing.py's shape table: Llama-3-8B (32 / 8
   heads, D = 128) and Llama-3.2-1B (32 / 8 heads, D = 64), q bf16, R in {29, 65}, prefix in {512, 2048, 8192},
   B in {1, 8}.  The two alternate in one process, device events around each block of steps after a warm-up,
   the median of the trials (microseconds per call, the Python wrapper included).  Beside every ratio stands the
   16-bit kernel's own trial spread ((max - min) / median): a ratio inside it says nothing.
2. ops.kv_store_fp8 (one launch for K and V) against the torch expression for both tensors,
   ``cache[:, :, pos:pos + R] = (x.float() / scale).clamp(-448, 448).to(float8_e4m3fn)``, at [1, 8, 29, 128] and
   [8, 8, 65, 128].

Writes profiles/tree_attention_fp8_timing.json.
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

HBM_PEAK = 8.0e12
MODELS = {"Llama-3-8B": (32, 8, 128), "Llama-3.2-1B": (32, 8, 64)}
F8 = torch.float8_e4m3fn


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def alternate(calls, steps, trials):
    """{name: trial times in us}: a warm-up, then `trials` rounds in which the candidates take turns."""
    for _ in range(10):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in calls}
    for _ in range(trials):
        for name, fn in calls.items():
            us[name].append(round(timed(fn, steps), 2))
    return us


def attention_table(steps, trials):
    from specdec_amd import ops
    dev, rows = "cuda", []
    for model, (Hq, Hkv, D) in MODELS.items():
        for B in (1, 8):
            for prefix in (512, 2048, 8192):
                for R in (29, 65):
                    g = torch.Generator().manual_seed(0)
                    L = prefix + R
                    q = torch.randn(B, Hq, R, D, generator=g).to(torch.bfloat16).to(dev)
                    k8, v8 = (torch.randn(B, Hkv, L, D, generator=g).to(dev).to(F8) for _ in range(2))
                    ks = (0.5 + 0.37 * torch.arange(Hkv)).to(dev)
                    vs = (1.25 - 0.11 * torch.arange(Hkv)).to(dev)
                    # the 16-bit call reads the dequantised cache: the same numbers, so the outputs compare
                    k16, v16 = ((t.float() * s[None, :, None, None]).to(torch.bfloat16) for t, s in ((k8, ks), (v8, vs)))
                    limit = torch.full((B, R), prefix + 1, dtype=torch.int32, device=dev)
                    words = [0] + [(1 << (i + 1)) - 1 for i in range(R - 1)]
                    bits = torch.tensor([[w - (1 << 64) if w >> 63 else w for w in words]] * B, device=dev)
                    calls = {"fp8": lambda: ops.tree_attention(q, k8, v8, limit, bits, prefix + 1, k_scale=ks, v_scale=vs),
                             "bf16": lambda: ops.tree_attention(q, k16, v16, limit, bits, prefix + 1)}
                    diff = float((calls["fp8"]().float() - calls["bf16"]().float()).abs().max())
                    us = alternate(calls, steps, trials)
                    med = {name: statistics.median(t) for name, t in us.items()}
                    kv_bytes = 2 * B * Hkv * L * D
                    rows.append(dict(model=model, B=B, prefix=prefix, R=R, splits=ops.tree_attention_splits(B, Hkv, L),
                                     max_abs_diff_to_bf16_of_rounded_cache=diff, trials_us=us, median_us=med,
                                     fp8_kv_bytes=kv_bytes,
                                     fp8_hbm_fraction=round(kv_bytes / (med["fp8"] * 1e-6) / HBM_PEAK, 4),
                                     bf16_spread=round((max(us["bf16"]) - min(us["bf16"])) / med["bf16"], 3),
                                     ratio_bf16_over_fp8=round(med["bf16"] / med["fp8"], 3)))
                    print(json.dumps(rows[-1]), flush=True)
    return rows


def store_table(steps, trials):
    from specdec_amd import ops
    dev, rows = "cuda", []
    for B, H, R, D in ((1, 8, 29, 128), (8, 8, 65, 128)):
        g = torch.Generator().manual_seed(1)
        L, pos = 2048 + R, 2048
        kn, vn = (torch.randn(B, H, R, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
        kc, vc = (torch.zeros(B, H, L, D, dtype=torch.uint8, device=dev).view(F8) for _ in range(2))
        ks = (0.5 + 0.37 * torch.arange(H)).to(dev)
        vs = (1.25 - 0.11 * torch.arange(H)).to(dev)

        def torch_store():
            for x, c, s in ((kn, kc, ks), (vn, vc, vs)):
                c[:, :, pos:pos + R] = (x.float() / s[None, :, None, None]).clamp(-448, 448).to(F8)

        us = alternate({"kv_store_fp8": lambda: ops.kv_store_fp8(kn, vn, kc, vc, ks, vs, pos), "torch": torch_store},
                       steps, trials)
        med = {name: statistics.median(t) for name, t in us.items()}
        rows.append(dict(shape=[B, H, R, D], trials_us=us, median_us=med,
                         ratio_torch_over_kernel=round(med["torch"] / med["kv_store_fp8"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_attention_fp8_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_attention_fp8_timing.py measures on the GPU; none found")
    res = dict(device=torch.cuda.get_device_name(0), q_dtype="bf16", steps=args.steps, trials=args.trials,
               hbm_peak_bytes_per_s=HBM_PEAK)
    res["attention"] = attention_table(args.steps, args.trials)
    res["store"] = store_table(args.steps, args.trials)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
