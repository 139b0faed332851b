"""Generate the golden vectors of the base decoders (sampling/base_decoding.py).

Run in the build container (where /root/reference exists), on the CPU:

    python tests/golden/make_golden_base.py

It imports the REFERENCE itself (read-only, with make_golden.py's stub for ``termcolor``), drives
``beam_search_generate`` and ``autoregressive_generate`` with the FakeLM banks of tests/fakelm.py and
writes ``beam_loops.json`` and ``ar_loops.json``: case parameters, bank digests and the reference's
returned tokens.  Only data is committed; the GPU box never runs this script.

Beam cases also carry, per step, the reference's own ``beams_probs`` bit patterns and
``last_indexes`` (read from its frame when it calls the model), and the margins that decide whether a
case may be held to the reference or only to tests/beam_ref.py:

* ``min_row_gap``     smallest non-zero gap inside the top-(k+1) float64 log-probs of a row fed to a step
* ``row_ties``        exact ties inside those top-(k+1) (equal logits: a tie in any arithmetic)
* ``min_score_gap``   smallest non-zero gap among a step's top num_beams+1 scores; ``score_ties`` the zero gaps
* ``aliasing_steps``  steps where the view semantics of beams_probs / last_indexes changed the state
* ``carried_steps``   steps entered with both a finished and a live beam
* ``min_boundary``    16-bit: smallest distance of a top-(k+1) float64 log-prob to a rounding boundary
* ``logsoftmax_err``  max |torch fp32 log_softmax - float64| over those values; ``bound`` = max(4 E, 2 fp32
                      ulps at the largest magnitude), E the largest logsoftmax_err of the row's size
                      class (cases of up to 4096 entries / all cases) — the figure tests/test_gpu_beam.py uses
* ``copy_visible``    a restatement with COPIES of a finished beam's score / last index differs from the
                      reference in the tokens or in a state that a later step reads
* ``tie_rule_matches``  tests/beam_ref.py (lowest index first, view semantics) reproduces the reference's
                      tokens and every recorded step state
* ``equal_reference`` the admission rule: margins >= 32 x bound, no exact tie in a 32-bit case, and
                      tie_rule_matches
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference, make_processor, prompt_for   # noqa: E402
from fakelm import make_pair, bank_digest, likely_tokens                # noqa: E402
import beam_ref                                                          # noqa: E402

DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
LIKELY3 = dict(rows=3, top=1, offset=0)

BEAM_CASES = [
    # name, V, dtype, num_beams, top_k, max_gen_len, eos ([..] | "likely" | "likely3"), seeds[, prompt]
    ("v4096_fp32_b4k3", 4096, "fp32", 4, 3, 24, [1], [1, 2, 3, 4, 5]),
    ("llama_fp32_b4k3", 128256, "fp32", 4, 3, 10, [1], [2, 3]),
    ("alias_fp32_b4k3", 4096, "fp32", 4, 3, 24, "likely3", [4], [5, 9, 2, 81]),
    ("alias_fp32_b4k3_p8", 4096, "fp32", 4, 3, 24, "likely3", [1, 2, 5, 7, 8, 9, 12]),
    ("carry_fp32_b6k4", 2048, "fp32", 6, 4, 30, "likely3", [0]),
    ("v4096_bf16_b4k3", 4096, "bf16", 4, 3, 24, [1], [0, 1, 2, 3]),
    ("v4096_bf16_b8k5", 4096, "bf16", 8, 5, 24, [1], [0, 1, 2, 3]),
    ("v4096_bf16_b4k3_eos", 4096, "bf16", 4, 3, 24, "likely", [0, 1, 2, 3]),
    ("v4096_bf16_b8k5_eos", 4096, "bf16", 8, 5, 24, "likely", [0, 1, 2, 3]),
    ("gen1_fp32_b4k3", 4096, "fp32", 4, 3, 1, [1], [1]),
    ("single_fp32_b1k1", 4096, "fp32", 1, 1, 16, [1], [1]),
    ("v4096_fp16_b4k3", 4096, "fp16", 4, 3, 16, [1], [1]),
]

AR_PROCS = [("greedy", 1.0, 0, 1.0), ("multinomial", 1.0, 0, 1.0), ("multinomial", 0.7, 0, 1.0),
            ("topk", 1.0, 20, 1.0), ("nucleus", 1.0, 0, 0.9)]


class SpyLM:
    """FakeLM that records, at every call after the first, what the calling loop holds in
    ``beams_probs`` / ``last_indexes`` (the state after the previous step)."""

    def __init__(self, lm):
        self.lm, self.config, self.states, self.calls = lm, lm.config, [], 0

    device = property(lambda self: self.lm.device)

    def __call__(self, *a, **k):
        loc = sys._getframe(1).f_locals
        if self.calls and "beams_probs" in loc:
            self.states.append(dict(bp=beam_ref.bits(loc["beams_probs"]), li=loc["last_indexes"].tolist()))
        self.calls += 1
        return self.lm(*a, **k)


def boundary_distance(v64: torch.Tensor, dtype) -> float:
    """Smallest distance of the float64 values to a round-to-nearest boundary of dtype."""
    r = v64.to(dtype)
    inf = torch.tensor(float("inf"), dtype=dtype)
    up, dn = torch.nextafter(r, inf).double(), torch.nextafter(r, -inf).double()
    r = r.double()
    return float(torch.minimum((v64 - (r + up) / 2).abs(), (v64 - (r + dn) / 2).abs()).min())


def margins_topk(rec, dt):
    """beam_ref's top-k with the margins of every row it is handed recorded into rec."""
    def fn(logits, k):
        x64 = logits.double()
        lp64 = torch.log_softmax(x64, dim=-1)
        kk = min(k + 1, logits.shape[-1])
        top = torch.sort(lp64, dim=-1, descending=True).values[..., :kk]
        gaps = top[..., :-1] - top[..., 1:]
        nz = gaps[gaps > 0]
        rec["min_row_gap"] = min(rec["min_row_gap"], float(nz.min()) if nz.numel() else float("inf"))
        rec["row_ties"] += int((gaps == 0).sum())
        lp32 = torch.log_softmax(logits.float(), dim=-1).double()
        top32 = torch.gather(lp32, -1, torch.sort(lp64, dim=-1, descending=True).indices[..., :kk])
        rec["logsoftmax_err"] = max(rec["logsoftmax_err"], float((top32 - top).abs().max()))
        rec["max_mag"] = max(rec["max_mag"], float(top.abs().max()))
        if dt != "fp32":
            rec["min_boundary"] = min(rec["min_boundary"], boundary_distance(top, DT[dt]))
        return beam_ref.logprob_topk(logits, k)
    return fn


def ulp32(x: float) -> float:
    t = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)


def eos_of(eos, target):
    if eos == "likely":
        return likely_tokens(target)
    if eos == "likely3":
        return likely_tokens(target, **LIKELY3)
    return eos


def make_beam(ref_beam):
    out = {}
    for name, V, dt, n, k, gen, eos_spec, seeds, *pr in BEAM_CASES:
        for seed in seeds:
            target, _ = make_pair(V, seed=seed, dtype=DT[dt])
            eos = eos_of(eos_spec, target)
            prompt = pr[0] if pr else prompt_for(V, seed)[0].tolist()
            spy = SpyLM(target)
            kw = dict(max_gen_len=gen, num_beams=n, top_k=k, eos_tokens_id=eos if len(eos) > 1 else eos[0],
                      pad_token_id=0)
            tokens = ref_beam(prompt, spy, **kw)
            rec = dict(min_row_gap=float("inf"), row_ties=0, logsoftmax_err=0.0, max_mag=0.0, min_boundary=float("inf"))
            trace = []
            mine = beam_ref.beam_search(prompt, target, trace=trace, topk_fn=margins_topk(rec, dt), **kw)
            states_equal = [dict(bp=t["bp"], li=t["li"]) for t in trace] == spy.states
            steps = [t for t in trace if "score_gap" in t]
            rec["min_score_gap"] = min([t["score_gap"] for t in steps], default=float("inf"))
            rec["score_ties"] = sum(t["score_ties"] for t in steps)
            rec["aliasing_steps"] = sum(1 for t in steps if t["aliasing"])
            rec["carried_steps"] = sum(t["carried"] for t in steps)
            rec["tie_rule_matches"] = bool(mine == tokens and states_equal)
            ctrace = []
            copy_tokens = beam_ref.beam_search(prompt, target, copy_semantics=True, trace=ctrace, **kw)
            rec["copy_semantics_differs"] = copy_tokens != tokens
            # the copy variant's difference as a caller can see it: in the tokens, or in a state a later step reads
            rec["copy_visible"] = copy_tokens != tokens or [dict(bp=t["bp"], li=t["li"]) for t in ctrace] != spy.states
            out[f"{name}/s{seed}"] = dict(
                vocab=V, dtype=dt, num_beams=n, top_k=k, max_gen_len=gen, eos=eos, seed=seed, prompt=prompt,
                min_length=5.0, alpha=1.2, target_digest=bank_digest(target), tokens=tokens, steps=spy.states, **rec)
    # The bound, as tests/test_gpu_beam.py applies it: torch's fp32 error E of the row's size class (the
    # largest logsoftmax_err over the cases of up to 4096 entries for those, over all cases beyond).
    inf = float("inf")
    e_small = max(c["logsoftmax_err"] for c in out.values() if c["vocab"] <= 4096)
    e_all = max(c["logsoftmax_err"] for c in out.values())
    for key, rec in out.items():
        rec["bound"] = max(4 * (e_small if rec["vocab"] <= 4096 else e_all), 2 * ulp32(rec["max_mag"]))
        need = 32 * rec["bound"]
        if rec["dtype"] == "fp32":
            ok = rec["min_row_gap"] >= need and rec["min_score_gap"] >= need and not rec["row_ties"] \
                and not rec["score_ties"]
        else:   # the rounded log-probs decide everything once they round the same way
            ok = rec["min_row_gap"] >= need and rec["min_boundary"] >= need
        rec["equal_reference"] = bool(ok and rec["tie_rule_matches"])
        print(key, len(rec["tokens"]), {a: rec[a] for a in ("equal_reference", "tie_rule_matches", "aliasing_steps",
                                                            "carried_steps", "row_ties", "min_row_gap", "min_score_gap",
                                                            "min_boundary", "bound", "copy_visible")}, flush=True)
        for m in ("min_row_gap", "min_score_gap", "min_boundary"):
            if rec[m] == inf:
                rec[m] = None
    eq = [v for v in out.values() if v["equal_reference"]]
    print("equal-the-reference:", len(eq), "with aliasing:", sum(1 for v in eq if v["aliasing_steps"]),
          "carrying >= 3 steps:", sum(1 for v in eq if v["carried_steps"] >= 3))
    assert len(eq) >= 12 and sum(1 for v in eq if v["aliasing_steps"]) >= 2 \
        and sum(1 for v in eq if v["carried_steps"] >= 3) >= 2 and sum(1 for v in eq if v["copy_visible"]) >= 2
    with open(os.path.join(HERE, "beam_loops.json"), "w") as f:
        json.dump(out, f, indent=1)


def rng_digest() -> str:
    return hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16]


def make_ar(ref_ar, lp):
    out = {}
    cases = [(4096, dt, proc, cache, eos) for dt in ("bf16", "fp32") for proc in AR_PROCS for cache in (False, True)
             for eos in ([1], "likely")]
    cases.append((128256, "bf16", AR_PROCS[1], False, [128001, 128009]))
    for V, dt, (kind, T, k, p), cache, eos_spec in cases:
        seed = 1
        target, _ = make_pair(V, dtype=DT[dt])
        eos = eos_of(eos_spec, target)
        prompt = prompt_for(V, seed)[0].tolist()
        torch.manual_seed(seed)
        tokens = ref_ar(prompt, target, max_gen_len=24 if V == 4096 else 8,
                        logits_processor=make_processor(lp, kind, T, k, p),
                        eos_tokens_id=eos if len(eos) > 1 else eos[0], pad_token_id=0, use_cache=cache)
        name = f"ar_v{V}_{dt}_{kind}_t{T}_{'cache' if cache else 'nocache'}_{'eos' if eos_spec == 'likely' else 'plain'}"
        out[name] = dict(vocab=V, dtype=dt, processor=dict(kind=kind, temperature=T, top_k=k, top_p=p),
                         use_cache=cache, eos=eos, seed=seed, prompt=prompt, max_gen_len=24 if V == 4096 else 8,
                         target_digest=bank_digest(target), tokens=tokens, rng_digest=rng_digest())
        print(name, len(tokens), flush=True)
    with open(os.path.join(HERE, "ar_loops.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    _, lp, _, _ = _import_reference()
    from sampling.base_decoding import autoregressive_generate, beam_search_generate   # the reference's
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    make_beam(beam_search_generate)
    make_ar(autoregressive_generate, lp)
