"""What the vocabulary-parallel verify costs on one rank.

    python scripts/vocab_parallel_timing.py [--steps 300] [--trials 5] [--out FILE]

BASELINE.json configs[4]'s verify shape (B = 1, γ = 4, V = 128256, bf16, multinomial) at S = 8: ONE
shard's three calls (sd_vp_stats, sd_vp_decide, sd_vp_finish on its 16032-column slices, with the
gathered blocks of a LocalShards step standing in for the exchanges, which are not timed) against
sd_verify(SD_RULE_SPEC) on the whole rows, alternating in one process (device events around each
block of steps after a warm-up; microseconds per step), and B = 16 likewise.  LocalShards is a
single-GPU emulation: no collective runs here.

For kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/vocab_parallel_timing.py
--trials 1` (no counters in the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))

GAMMA, VOCAB, SHARDS = 4, 128256, 8


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def table(steps, trials):
    from specdec_amd import _lib, ops, vocab_parallel as vp
    from specdec_amd.noise import PhiloxNoise
    dev, spec = "cuda", ops.ProcSpec("multinomial", 1.0)
    ls = vp.LocalShards.even(SHARDS, VOCAB)
    rows = []
    for B in (1, 16):
        g = torch.Generator().manual_seed(B)
        tl = (torch.randn(B, GAMMA + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
        dl = (tl[:, :GAMMA].float() + torch.randn(B, GAMMA, VOCAB, generator=g).to(dev)).to(torch.bfloat16)
        tok = torch.randint(0, VOCAB, (B, GAMMA), generator=g).to(dev)
        tok[:, :2] = dl[:, :2].float().argmax(-1)                 # some accepts, then coin flips
        noise = PhiloxNoise(seed=1)
        nz, _ = ops._noise_struct(noise, 0, torch.device(dev), 0)
        steps_ = [vp._step_of(sh.view(tl), sh.view(dl), tok, spec, nz, sh) for sh in ls.shards]
        stats_all = ls.concat([st.stats() for st in steps_])
        cand_all = ls.concat([st.decide(stats_all) for st in steps_])
        mine = steps_[3]                                          # one rank's work

        def sharded():
            mine.stats()
            mine.decide(stats_all)
            mine.finish(cand_all)

        trows, drows = [tl[:, t] for t in range(GAMMA + 1)], [dl[:, t] for t in range(GAMMA)]

        def whole():
            ops.verify(trows, drows, tok, _lib.SD_RULE_SPEC, spec, spec, noise)

        for _ in range(20):
            sharded()
            whole()
        torch.cuda.synchronize()
        s, w = [], []
        for _ in range(trials):
            s.append(round(timed(sharded, steps), 2))
            w.append(round(timed(whole, steps), 2))
        rows.append(dict(B=B, vp_one_rank_us=s, sd_verify_whole_rows_us=w,
                         whole_path=_lib.PATH_NAMES[_lib.last_verify_path()],
                         exchange_bytes_per_rank=[int(stats_all.shape[1]), int(cand_all.shape[1])],
                         logit_bytes_not_gathered=B * (GAMMA + 1) * VOCAB * 2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), gamma=GAMMA, vocab=VOCAB, shards=SHARDS, dtype="bf16",
               steps=args.steps, trials=args.trials, rows=table(args.steps, args.trials))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
