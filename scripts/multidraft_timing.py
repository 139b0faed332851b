"""What the multi-draft verify costs.

    python scripts/multidraft_timing.py [--steps 500] [--trials 5] [--no-loop] [--no-verify] [--out FILE]

1. One sd_verify_multi at B = 1, γ = 4, V = 128256, bf16, K in {1, 2, 4, 8} against sd_verify(SD_RULE_SPEC)
   at B = K on the same K(2γ+1) rows, alternating in one process (device events around each block of
   steps after a warm-up; microseconds per call).
2. Tokens per second of multidraft_speculative_generate (K in {1, 2, 4}) against speculative_generate
   on a FakeLM pair (vocab 128256, bf16, multinomial, γ = 4): the loops' host and kernel time without
   model forwards to speak of, so the verify step's share is at its largest.

For kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/multidraft_timing.py --no-loop
--trials 1` (no counters in the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GAMMA, VOCAB = 4, 128256


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def verify_table(steps, trials):
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    dev, spec = "cuda", ops.ProcSpec("multinomial", 1.0)
    rows = []
    for K in (1, 2, 4, 8):
        g = torch.Generator().manual_seed(K)
        tl = (torch.randn(1, K, GAMMA + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
        dl = (tl[:, :, :GAMMA].float() + torch.randn(1, K, GAMMA, VOCAB, generator=g).to(dev)).to(torch.bfloat16)
        tok = torch.randint(0, VOCAB, (1, K, GAMMA), generator=g).to(dev)
        tok[0, :, :2] = dl[0, :, :2].float().argmax(-1)          # some accepts, then coin flips
        noise = PhiloxNoise(seed=1)
        trows, drows = [tl[0, :, t] for t in range(GAMMA + 1)], [dl[0, :, t] for t in range(GAMMA)]

        def multi():
            ops.verify_multi(tl, dl, tok, spec, noise)

        def single():
            ops.verify(trows, drows, tok[0], _lib.SD_RULE_SPEC, spec, spec, noise)

        for _ in range(20):
            multi()
            single()
        torch.cuda.synchronize()
        m, s = [], []
        for _ in range(trials):
            m.append(round(timed(multi, steps), 2))
            s.append(round(timed(single, steps), 2))
        rows.append(dict(K=K, verify_multi_us=m, sd_verify_B_eq_K_us=s, single_path=_lib.PATH_NAMES[_lib.last_verify_path()],
                         bytes_read=K * (2 * GAMMA + 1) * VOCAB * 2))
    return rows


def loop_table(trials, gen_len):
    import fakelm
    import specdec_amd
    from specdec_amd.sampling import multidraft_speculative_generate, speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = fakelm.make_pair(VOCAB, sigma=1.0, device="cuda")
    proc, prompt = MultinomialProcessor(1.0), list(range(3, 35))
    kw = dict(gamma=GAMMA, logits_processor=proc, max_gen_len=gen_len, eos_tokens_id=[VOCAB + 1])
    specdec_amd.set_noise_mode("philox", 7)

    def run(fn):
        fn()                                                     # warm-up (workspaces, caches)
        best = None
        for t in range(trials):
            torch.manual_seed(t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, rate = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r = dict(tokens_per_s=round(len(toks) / dt, 1), acceptance=round(float(rate), 3))
            best = r if best is None or r["tokens_per_s"] > best["tokens_per_s"] else best
        return best

    rows = [dict(loop="speculative_generate", **run(lambda: speculative_generate(prompt, drafter, target, **kw)))]
    for K in (1, 2, 4):
        rows.append(dict(loop=f"multidraft K={K}",
                         **run(lambda: multidraft_speculative_generate(prompt, drafter, target, num_drafts=K, **kw))))
    specdec_amd.set_noise_mode("stream")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--gen", type=int, default=256)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), gamma=GAMMA, vocab=VOCAB, dtype="bf16", steps=args.steps,
               trials=args.trials)
    if not args.no_verify:
        res["verify"] = verify_table(args.steps, args.trials)
    if not args.no_loop:
        res["loop"] = loop_table(args.trials, args.gen)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
