"""One beam-search step at the reference's defaults (num_beams = 4, top_k = 3) on [4, 128256] bf16
logits: the device step (one sd_beam_step: k_beam_topk + k_beam_select) against torch-ROCm running
the reference's own expression of the step (log_softmax, topk and the per-candidate loop of
sampling/base_decoding.py:136-178, restated below), alternating in one process.

    python scripts/beam_timing.py [--steps 2000] [--trials 5] [--out FILE] [--no-torch]

Device events around each block of steps, after a warm-up; microseconds per step (the stream's
elapsed time, so the host's launch cost shows where the stream runs dry).  --no-torch leaves only
the device step, for a separate `rocprofv3 --kernel-trace --stats -- python scripts/beam_timing.py
--no-torch --trials 1` run (kernel times; the row pass reads rows * vocab * 2 bytes).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))

N_BEAMS, TOP_K, VOCAB, PROMPT, TOTAL = 4, 3, 128256, 8, 48


def torch_step(logits, ids, probs, beams_probs, last, curr, lp, stops, pad):
    """The step as the reference expresses it: per candidate a few 0-dim tensor ops, a whole-row
    equality test against every earlier candidate, then a Python sort."""
    logp = torch.nn.functional.log_softmax(logits, dim=-1)
    top_p, top_t = torch.topk(logp, TOP_K, dim=-1)
    cands = []
    for b in range(N_BEAMS):
        if last[b] != -1:
            cands.append((beams_probs[b], ids[b].clone(), probs[b].clone(), last[b]))
            continue
        for j in range(TOP_K):
            total = probs[b, curr - 1] + top_p[b, j]
            prow = probs[b].clone()
            prow[curr] = total
            irow = ids[b].clone()
            irow[curr] = top_t[b, j]
            end = curr if (torch.isin(irow[curr], stops) or irow[curr] == pad) else -1
            if not any(torch.equal(c[1], irow) for c in cands):
                cands.append((total / lp, irow, prow, end))
    cands.sort(key=lambda c: c[0], reverse=True)
    for b in range(N_BEAMS):
        beams_probs[b] = cands[b][0]
        ids[b] = cands[b][1]
        probs[b] = cands[b][2]
        last[b] = cands[b][3]
    return torch.all(last != -1)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--torch-steps", type=int, default=0, help="steps per torch trial (default: --steps)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from specdec_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(N_BEAMS, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
    prompt = torch.randint(3, VOCAB, (PROMPT,), generator=g).tolist()
    stops = torch.tensor([1], dtype=torch.long, device=dev)
    curr = PROMPT + 4
    lp = ops.beam_length_penalty(curr - PROMPT, 1.2, 5.0)

    state = ops.BeamState.start(prompt, N_BEAMS, TOTAL, 0, dev)
    state.probs[:, PROMPT:curr] = -1.0

    def ours():
        ops.beam_step(state, logits, curr, top_k=TOP_K, length=curr - PROMPT, stop_tokens=stops, pad_token_id=0)

    ref = ops.BeamState.start(prompt, N_BEAMS, TOTAL, 0, dev)
    ref.probs[:, PROMPT:curr] = -1.0
    t_ids, t_probs = ref.input_ids.clone(), ref.probs.clone()
    t_bp, t_last = ref.beams_probs.clone(), ref.last_indexes.clone()

    def theirs():
        t_last.fill_(-1)   # every timed step expands all four beams
        torch_step(logits, t_ids, t_probs, t_bp, t_last, curr, lp, stops, 0)

    for _ in range(50):
        ours()
    if not args.no_torch:
        for _ in range(5):
            theirs()
    torch.cuda.synchronize()
    res = dict(shape=[N_BEAMS, VOCAB], dtype="bf16", num_beams=N_BEAMS, top_k=TOP_K, trials=args.trials,
               steps=args.steps, torch_steps=0 if args.no_torch else (args.torch_steps or args.steps),
               device=torch.cuda.get_device_name(0), beam_step_us=[], torch_step_us=[])
    for _ in range(args.trials):
        res["beam_step_us"].append(round(timed(ours, args.steps), 2))
        if not args.no_torch:
            res["torch_step_us"].append(round(timed(theirs, args.torch_steps or args.steps), 2))
    res["row_pass_bytes"] = N_BEAMS * VOCAB * 2
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
