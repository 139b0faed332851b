"""tests/beam_ref.py (the CPU restatement the device beam step is checked against) against the
reference's goldens (tests/golden/beam_loops.json): it reproduces every equal-the-reference case's
tokens and per-step state, and its copy-semantics variant does NOT on the aliasing cases — so the
fixtures exercise the reference's view aliasing of beams_probs / last_indexes."""
import json
import os

import pytest
import torch

import beam_ref
from fakelm import bank_digest, make_pair

HERE = os.path.dirname(os.path.abspath(__file__))
DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}
with open(os.path.join(HERE, "golden", "beam_loops.json")) as f:
    BEAM = json.load(f)
EQUAL = sorted(k for k, c in BEAM.items() if c["equal_reference"])


def run(c, **kw):
    target, _ = make_pair(c["vocab"], seed=c["seed"], dtype=DT[c["dtype"]])
    assert bank_digest(target) == c["target_digest"]
    eos = c["eos"]
    return beam_ref.beam_search(c["prompt"], target, max_gen_len=c["max_gen_len"], num_beams=c["num_beams"],
                                top_k=c["top_k"], min_length=c["min_length"], alpha=c["alpha"],
                                eos_tokens_id=eos if len(eos) > 1 else eos[0], pad_token_id=0, **kw)


def test_the_set_meets_the_admission_counts():
    eq = [BEAM[k] for k in EQUAL]
    assert len(eq) >= 12
    assert sum(1 for c in eq if c["aliasing_steps"]) >= 2
    assert sum(1 for c in eq if c["carried_steps"] >= 3) >= 2
    for c in eq:
        need = 32 * c["bound"]
        assert c["tie_rule_matches"]
        assert c["min_row_gap"] is None or c["min_row_gap"] >= need
        if c["dtype"] == "fp32":
            assert not c["row_ties"] and not c["score_ties"]
            assert c["min_score_gap"] is None or c["min_score_gap"] >= need
        else:
            assert c["min_boundary"] >= need
    assert "alias_fp32_b4k3/s4" in EQUAL and "carry_fp32_b6k4/s0" in EQUAL


@pytest.mark.parametrize("name", EQUAL)
def test_restatement_reproduces_the_reference(name):
    c = BEAM[name]
    trace = []
    assert run(c, trace=trace) == c["tokens"]
    assert [dict(bp=t["bp"], li=t["li"]) for t in trace] == c["steps"]


def test_enough_cases_show_the_aliasing():
    assert sum(1 for k in EQUAL if BEAM[k]["copy_visible"]) >= 2


@pytest.mark.parametrize("name", [k for k in EQUAL if BEAM[k]["copy_visible"]])
def test_copy_semantics_differ_on_the_aliasing_cases(name):
    c = BEAM[name]
    trace = []
    tokens = run(c, copy_semantics=True, trace=trace)
    states = [dict(bp=t["bp"], li=t["li"]) for t in trace]
    assert states != c["steps"][:len(states)] or len(states) != len(c["steps"]) or tokens != c["tokens"]


def test_the_issue_case_returns_other_tokens_with_copies():
    c = BEAM["alias_fp32_b4k3/s4"]
    assert c["copy_semantics_differs"] == (run(c, copy_semantics=True) != c["tokens"])
    assert any(BEAM[k]["copy_semantics_differs"] for k in EQUAL)


def test_lowest_index_first_topk():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, float("-inf")]])
    v, i = beam_ref.topk_lowest_index(x, 4)
    assert i.tolist() == [[1, 2, 4, 3]] and v.tolist() == [[3.0, 3.0, 3.0, 2.0]]
    lp, tok = beam_ref.logprob_topk(x.to(torch.bfloat16), 2)
    assert tok.tolist() == [[1, 2]] and lp.dtype == torch.float32
