"""What block verification costs and what it buys.

    python scripts/block_timing.py [--steps 300] [--trials 5] [--no-loop] [--no-verify] [--lib NAME] [--out FILE]

1. One sd_verify_block against one sd_verify(SD_RULE_SPEC, PHILOX) on the same rows: B = 1 and B = 32,
   γ = 4, V = 128256, bf16, multinomial and nucleus 0.9, alternating in one process (device events around
   each block of steps after a warm-up; microseconds per call).  Every shape is measured by a child
   process of its own under its own time limit (--shape-limit seconds), so one that hangs costs that
   shape alone.  --lib selects another in-tree build (SPECDEC_LIB), e.g. the weight-table variant.
2. Accepted drafts per verify step and tokens per target forward of block_speculative_generate against
   speculative_generate on the FakeLM pair of the loop tests (vocab 4096, sigma 1, multinomial), the
   same prompts and seeds, γ = 4 and 8, with the host model's expectation beside it
   (block_cases.simulate_acceptance).

For kernel times: `rocprofv3 --kernel-trace --stats -- python scripts/block_timing.py --no-loop --trials 1
--inline` (no counters in the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speculative-decoding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GAMMA, VOCAB = 4, 128256
SHAPES = [(B, name) for B in (1, 32) for name in ("multinomial", "nucleus0.9")]


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def verify_row(B, name, steps, trials):
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    dev = "cuda"
    spec = ops.ProcSpec("multinomial", 1.0) if name == "multinomial" else ops.ProcSpec("nucleus", 1.0, 0, 0.9)
    g = torch.Generator().manual_seed(B)
    tl = (torch.randn(B, GAMMA + 1, VOCAB, generator=g) * 3).to(torch.bfloat16).to(dev)
    dl = (tl[:, :GAMMA].float() + torch.randn(B, GAMMA, VOCAB, generator=g).to(dev)).to(torch.bfloat16)
    tok = torch.randint(0, VOCAB, (B, GAMMA), generator=g).to(dev)
    tok[:, :2] = dl[:, :2].float().argmax(-1)                    # some accepts, then coin flips
    noise = PhiloxNoise(seed=1)
    trows, drows = [tl[:, t] for t in range(GAMMA + 1)], [dl[:, t] for t in range(GAMMA)]

    def block():
        ops.verify_block(trows, drows, tok, spec, noise, want_tokens=False)

    def single():
        ops.verify(trows, drows, tok, _lib.SD_RULE_SPEC, spec, spec, noise)

    for _ in range(20):
        block()
        single()
    torch.cuda.synchronize()
    single()
    path = _lib.PATH_NAMES[_lib.last_verify_path()]
    bl, si = [], []
    for _ in range(trials):
        bl.append(round(timed(block, steps), 2))
        si.append(round(timed(single, steps), 2))
    return dict(B=B, proc=name, verify_block_us=bl, sd_verify_us=si, sd_verify_path=path,
                bytes_read=B * (2 * GAMMA + 1) * VOCAB * 2)


def verify_table(steps, trials, limit, inline):
    rows = []
    for B, name in SHAPES:
        if inline:
            rows.append(verify_row(B, name, steps, trials))
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(B), name, "--steps", str(steps), "--trials", str(trials)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            rows.append(dict(B=B, proc=name, error=f"no result within {limit} s"))
            break                                                # nothing more on the GPU after a hang
        if r.returncode != 0:
            rows.append(dict(B=B, proc=name, error=f"exit status {r.returncode}", stderr=r.stderr[-400:]))
            break
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    return rows


def loop_table(seeds, gen_len):
    import fakelm
    import block_cases as bc
    import specdec_amd
    from specdec_amd.sampling import block_speculative_generate, speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = fakelm.make_pair(4096, sigma=1.0, device="cuda")
    calls = [0]

    class Counting(fakelm.FakeLM):
        def __call__(self, **kw):
            calls[0] += 1
            return super().__call__(**kw)

    counted = Counting(target.bank)
    proc, prompt = MultinomialProcessor(1.0), [5, 17, 101, 9, 2000, 77]
    rows = []
    for gamma in (4, 8):
        kw = dict(gamma=gamma, logits_processor=proc, max_gen_len=gen_len, eos_tokens_id=[4096 + 5])
        res = {}
        for name in ("speculative_generate", "block_speculative_generate"):
            toks = fwd = 0
            rate = 0.0
            for s in range(seeds):
                torch.manual_seed(s)
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                torch.manual_seed(s)
                calls[0] = 0
                if name == "speculative_generate":
                    specdec_amd.set_noise_mode("philox", seed)
                    out, r = speculative_generate(prompt, drafter, counted, **kw)
                    specdec_amd.set_noise_mode("stream")
                else:
                    out, r = block_speculative_generate(prompt, drafter, counted, **kw)
                toks, fwd, rate = toks + len(out), fwd + calls[0], rate + float(r)
            res[name] = dict(tokens_per_target_forward=round(toks / fwd, 4), accepted_per_step=round(rate / seeds * gamma, 4))
        cpu_t, cpu_d = fakelm.make_pair(4096, sigma=1.0)
        host = {("block" if blk else "tokenwise"): round(sum(bc.simulate_acceptance(cpu_t, cpu_d, gamma, 300, s, block=blk)
                                                             for s in range(3)) / 3, 4) for blk in (True, False)}
        rows.append(dict(gamma=gamma, seeds=seeds, gen_len=gen_len, **res, host_model_accepted_per_step=host))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--gen", type=int, default=256)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--shape-limit", type=int, default=120)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--inline", action="store_true", help="measure every shape in this process (for a profiler)")
    ap.add_argument("--one", nargs=2, metavar=("B", "PROC"), help="measure one shape and print its row")
    ap.add_argument("--lib", help="another in-tree build of the library (file name under specdec_amd/)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.lib:
        os.environ["SPECDEC_LIB"] = args.lib
    if args.one:
        print(json.dumps(verify_row(int(args.one[0]), args.one[1], args.steps, args.trials)))
        return
    res = dict(device=torch.cuda.get_device_name(0), gamma=GAMMA, vocab=VOCAB, dtype="bf16", steps=args.steps,
               trials=args.trials, lib=os.environ.get("SPECDEC_LIB", "libspecdec.so"))
    if not args.no_verify:
        res["verify"] = verify_table(args.steps, args.trials, args.shape_limit, args.inline)
    if not args.no_loop:
        res["loop"] = loop_table(args.seeds, args.gen)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
