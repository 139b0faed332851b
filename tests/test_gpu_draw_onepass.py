"""k_draw_lean's tail wave with one lane pass (rows of at most 64 spans; csrc/specdec_kernels.hip, the
kernel's NP parameter): the multinomial draw with row statistics and token_prob on B = 3 rows of bf16 and
fp16, at V in {8, 2048, 2056, 129024, 131072} — 1, 1, 2, 63 and 64 spans of 2048 elements, the last the
largest row that takes one pass — contiguous and at a padded 16-byte stride.

Two checks per case, and every case asserts the kernel it ran (_lib.last_sample_path()):
  * the tokens against the fp64 host model of the draw (tests/draw_ref.py), with the checker and the caps
    of tests/test_gpu_draw_exact.py (hold);
  * every output — tokens, token_prob, the row statistics (max, sum of exponentials) and the row status —
    bit for bit against tests/golden/draw_onepass.json, which tests/golden/make_draw_onepass.py wrote
    from the library of the commit before the pass count became a parameter (two passes for every row).

The greedy draw keeps its two passes (launch_draw_lean_t), so it has no case here."""
import json
import os

import pytest
import torch

import draw_cases as dc
import draw_ref as dr
import row_edges as re_

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_onepass.json")
VOCABS = (8, 2048, 2056, 129024, 131072)
SPANS = {8: 1, 2048: 1, 2056: 2, 129024: 63, 131072: 64}
OFFSETS = (3, (1 << 33) + 5)
ROW_BASES = (0, 70001)


def cases():
    return [dc._case("lean", 3, V, dt, layout=layout, offsets=OFFSETS, row_bases=ROW_BASES)
            for dt in (dc.BF16, dc.F16) for V in VOCABS for layout in ("contiguous", "padded")]


def lib():
    from types import SimpleNamespace
    from specdec_amd import PhiloxNoise, _lib, ops
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise)


def run_case(sd, c):
    """The case's draws: per offset {tokens, prob (bits), stats (bits), status}; asserts the path."""
    x, kinds = dc.case_rows(c)
    assert (c.V + 2047) // 2048 == SPANS[c.V] <= 64
    rows = dc.place(x, c.layout, DEV)
    assert re_.rows_aligned(rows) and (c.layout == "contiguous" or rows.stride(0) > c.V)
    spec = sd.ops.ProcSpec("multinomial", 1.0)
    out = []
    for off, rb in zip(c.offsets, c.row_bases):
        stats = torch.full((c.B, 2), float("nan"), device=DEV)
        tok, prob, st = sd.ops.sample_rows(rows, spec, sd.PhiloxNoise(seed=c.noise_seed, offset=off), want_prob=True,
                                           row_base=rb, row_stats_out=stats)
        assert sd.lib.last_sample_path() == sd.lib.SD_PATH_SAMPLE_DRAW_LEAN, sd.lib.PATH_NAMES.get(sd.lib.last_sample_path())
        out.append({"tokens": tok.cpu().tolist(), "prob": prob.cpu().view(torch.int32).tolist(),
                    "stats": stats.cpu().view(torch.int32).flatten().tolist(), "status": st.cpu().tolist()})
    return x, kinds, out


def run_all(sd):
    return {c.id: run_case(sd, c)[2] for c in cases()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("c", cases(), ids=lambda c: c.id)
def test_one_pass_tail_draws_the_models_token_and_the_two_pass_outputs(c, golden):
    from test_gpu_draw_exact import hold
    sd = lib()
    x, kinds, out = run_case(sd, c)
    for o in out:
        st = torch.tensor(o["status"])
        assert bool(((st & sd.lib.SD_ROW_DONE) != 0).all()) and not bool((st & sd.lib.SD_ROW_ERROR_MASK).any()), o["status"]
    tabs = [dr.lean_tables(x[r], c.dtype, 1) for r in range(c.B)]
    hold(c, "k_draw_lean", ((f"off={off} row={r} ({kinds[r]})", tabs[r], dr.lean_row(tabs[r], c.noise_seed, off, rb + r),
                             out[i]["tokens"][r], dr.check_lean)
                            for i, (off, rb) in enumerate(zip(c.offsets, c.row_bases)) for r in range(c.B)))
    assert out == golden[c.id], (c.id, out, golden[c.id])
