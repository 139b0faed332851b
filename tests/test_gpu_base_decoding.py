"""autoregressive_generate and beam_search_generate on the GPU against the reference's goldens
(tests/golden/beam_loops.json, ar_loops.json; made by tests/golden/make_golden_base.py).

A beam case is held to the reference's tokens when its recorded margins admit it
(``equal_reference``); the others — bf16 rows whose equal log-probs torch.topk orders its own way,
or margins too thin for any arithmetic but the reference's — are held to tests/beam_ref.py.
"""
import hashlib
import json
import os

import pytest
import torch

import beam_ref
from fakelm import bank_digest, make_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
with open(os.path.join(HERE, "golden", "beam_loops.json")) as f:
    BEAM = json.load(f)
with open(os.path.join(HERE, "golden", "ar_loops.json")) as f:
    AR = json.load(f)

_banks = {}


def target_for(V, seed, dt):
    """(CPU FakeLM, GPU FakeLM) of a bank, made once per (V, seed, dtype)."""
    key = (V, seed, dt)
    if key not in _banks:
        cpu, _ = make_pair(V, seed=seed, dtype=DT[dt])
        _banks[key] = (cpu, cpu.to(DEV))
    return _banks[key]


def beam_kwargs(c):
    eos = c["eos"]
    return dict(max_gen_len=c["max_gen_len"], num_beams=c["num_beams"], top_k=c["top_k"], min_length=c["min_length"],
                alpha=c["alpha"], eos_tokens_id=eos if len(eos) > 1 else eos[0], pad_token_id=0)


@pytest.mark.parametrize("name", sorted(BEAM))
def test_beam_search_generate_equals_golden(name):
    from specdec_amd.sampling import beam_search_generate
    c = BEAM[name]
    cpu, gpu = target_for(c["vocab"], c["seed"], c["dtype"])
    assert bank_digest(cpu) == c["target_digest"]
    got = beam_search_generate(c["prompt"], gpu, **beam_kwargs(c))
    if c["equal_reference"]:
        assert got == c["tokens"]
    else:
        assert got == beam_ref.beam_search(c["prompt"], cpu, **beam_kwargs(c))


def test_golden_set_is_what_the_admission_rule_needs():
    eq = [c for c in BEAM.values() if c["equal_reference"]]
    assert len(eq) >= 12
    assert sum(1 for c in eq if c["aliasing_steps"]) >= 2
    assert sum(1 for c in eq if c["carried_steps"] >= 3) >= 2


def test_beam_search_reads_one_word_per_step(monkeypatch):
    from specdec_amd.sampling import beam_search_generate
    c = BEAM["v4096_fp32_b4k3/s1"]
    _, gpu = target_for(c["vocab"], c["seed"], c["dtype"])
    events = []

    class Spy:
        config, device = gpu.config, gpu.device

        def __call__(self, *a, **k):
            events.append("model")
            return gpu(*a, **k)

    for meth in ("item", "tolist", "cpu"):
        orig = getattr(torch.Tensor, meth)

        def wrapped(self, *a, _orig=orig, **k):
            if self.is_cuda:
                events.append("read")
            return _orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, meth, wrapped)
    got = beam_search_generate(c["prompt"], Spy(), **beam_kwargs(c))
    monkeypatch.undo()
    assert got == c["tokens"]
    steps = "".join("M" if e == "model" else "r" for e in events).split("M")[1:]
    assert len(steps) == c["max_gen_len"]
    assert all(len(s) <= 1 for s in steps[:-1]), steps          # one read per step at the most
    assert len(steps[-1]) <= 3                                   # the last step's, then the result's two


def test_beam_search_argument_errors():
    from specdec_amd.sampling import beam_search_generate
    cpu, gpu = target_for(4096, 1, "fp32")
    with pytest.raises(IndexError):
        beam_search_generate([5, 9, 2], gpu, max_gen_len=0)
    with pytest.raises(RuntimeError):
        beam_search_generate([5, 9, 2], gpu, max_gen_len=4, top_k=5000)
    with pytest.raises(RuntimeError):
        beam_search_generate([5, 9, 2], gpu, max_gen_len=4, num_beams=5000, top_k=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        beam_search_generate([5, 9, 2], cpu, max_gen_len=4)


def make_processor(kind, T, k, p):
    from specdec_amd.utils import logits_processor as lp
    return {"greedy": lambda: lp.GreedyProcessor(T), "multinomial": lambda: lp.MultinomialProcessor(T),
            "topk": lambda: lp.TopKProcessor(T, k), "nucleus": lambda: lp.NucleusProcessor(T, p)}[kind]()


@pytest.mark.parametrize("name", sorted(AR))
def test_autoregressive_generate_equals_golden(name):
    from specdec_amd import noise
    from specdec_amd.sampling import autoregressive_generate
    c = AR[name]
    cpu, gpu = target_for(c["vocab"], 0, c["dtype"])
    assert bank_digest(cpu) == c["target_digest"]
    p = c["processor"]
    eos = c["eos"]
    noise.set_noise_mode("stream")   # the parity mode (the default): torch's CPU generator words
    torch.manual_seed(c["seed"])
    got = autoregressive_generate(c["prompt"], gpu, max_gen_len=c["max_gen_len"],
                                  logits_processor=make_processor(p["kind"], p["temperature"], p["top_k"], p["top_p"]),
                                  eos_tokens_id=eos if len(eos) > 1 else eos[0], pad_token_id=0,
                                  use_cache=c["use_cache"])
    assert got == c["tokens"]
    assert hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16] == c["rng_digest"]


def test_autoregressive_generate_refuses_what_the_loops_refuse():
    from specdec_amd.sampling import autoregressive_generate
    from specdec_amd.utils.logits_processor import GreedyProcessor
    cpu, gpu = target_for(4096, 0, "bf16")

    class Sampler(GreedyProcessor):
        def sample(self, probs):
            return probs.argmax(-1)

    with pytest.raises(TypeError):
        autoregressive_generate([5, 9, 2], gpu, max_gen_len=4, logits_processor=Sampler())
    with pytest.raises(RuntimeError, match="no CPU path"):
        autoregressive_generate([5, 9, 2], cpu, max_gen_len=4)


def test_autoregressive_generate_runs_a_user_process_override():
    """A subclass's own _process runs as written (ops.processed_rows): banning the greedy token moves
    the first pick to the runner-up."""
    from specdec_amd.sampling import autoregressive_generate
    from specdec_amd.utils.logits_processor import GreedyProcessor
    _, gpu = target_for(4096, 0, "bf16")
    plain = autoregressive_generate([5, 9, 2], gpu, max_gen_len=3)

    class Banned(GreedyProcessor):
        def _process(self, logits):
            logits[..., plain[0]] = -1e20
            return logits

    got = autoregressive_generate([5, 9, 2], gpu, max_gen_len=3, logits_processor=Banned())
    assert got[0] != plain[0]
