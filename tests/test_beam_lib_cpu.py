"""CPU-side checks of the beam step's C ABI (ABI 12): the ctypes mirror of sd_beam_args has the C
layout, the package exports the two decoders, and sd_beam_step refuses bad arguments before it
touches a device."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "specdec.h")

C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "specdec.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("sd_beam_args %zu\n", sizeof(sd_beam_args));
  printf("sd_verify_args %zu\n", sizeof(sd_verify_args));
  printf("sd_sample_args %zu\n", sizeof(sd_sample_args));
  printf("sd_ngram_args %zu\n", sizeof(sd_ngram_args));
  F(sd_beam_args, lp) F(sd_beam_args, logits) F(sd_beam_args, dtype) F(sd_beam_args, stop_tokens)
  F(sd_beam_args, pad_token) F(sd_beam_args, input_ids_stride) F(sd_beam_args, probs_stride)
  F(sd_beam_args, last_index_out) F(sd_beam_args, top_logprob) F(sd_beam_args, all_finished)
  F(sd_beam_args, parent) F(sd_beam_args, workspace_bytes)
  printf("abi %d\n", SD_ABI_VERSION);
  printf("limits %d\n", SD_BEAM_MAX_BEAMS * 1000000 + SD_BEAM_MAX_TOPK * 10000 + SD_BEAM_MAX_CANDIDATES);
  return 0;
}
"""


def test_ctypes_layout_matches_c_header_and_abi_is_12():
    from specdec_amd import _lib
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(C_LAYOUT)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line)
    assert int(got["sd_beam_args"]) == C.sizeof(_lib.sd_beam_args)
    for key, val in got.items():
        if "." in key:
            struct, field = key.split(".")
            assert getattr(getattr(_lib, struct), field).offset == int(val), key
    assert int(got["abi"]) == 12 == _lib.SD_ABI_VERSION == _lib.lib.sd_abi_version()
    assert int(got["limits"]) == _lib.SD_BEAM_MAX_BEAMS * 1000000 + _lib.SD_BEAM_MAX_TOPK * 10000 \
        + _lib.SD_BEAM_MAX_CANDIDATES
    # the existing structs keep their sizes (ABI 11's)
    assert (int(got["sd_verify_args"]), int(got["sd_sample_args"]), int(got["sd_ngram_args"])) == \
        (C.sizeof(_lib.sd_verify_args), C.sizeof(_lib.sd_sample_args), C.sizeof(_lib.sd_ngram_args)) == (888, 184, 488)


def test_sampling_exports_the_reference_names():
    import inspect
    import specdec_amd.sampling as s
    for name in ("autoregressive_generate", "beam_search_generate", "speculative_generate", "max_fn"):
        assert callable(getattr(s, name)), name
    p = inspect.signature(s.beam_search_generate).parameters
    assert list(p) == ["inputs", "model", "max_gen_len", "num_beams", "top_k", "min_length", "alpha",
                       "eos_tokens_id", "pad_token_id", "debug", "tokenizer"]
    assert [p[k].default for k in list(p)[2:]] == [40, 4, 3, 5.0, 1.2, 1, 0, False, None]
    p = inspect.signature(s.autoregressive_generate).parameters
    assert list(p) == ["inputs", "model", "max_gen_len", "logits_processor", "eos_tokens_id", "pad_token_id",
                       "use_cache", "debug"]
    assert [p[k].default for k in ("max_gen_len", "eos_tokens_id", "pad_token_id", "use_cache", "debug")] == \
        [40, 1, 0, False, False]


def _valid_step():
    from specdec_amd import _lib
    a = _lib.sd_beam_args()
    a.mode, a.num_beams, a.top_k, a.vocab, a.curr, a.total_len, a.lp = _lib.SD_BEAM_STEP, 4, 3, 4096, 5, 16, 1.25
    a.logits, a.stride_r, a.dtype = 0x100000, 4096, _lib.SD_BF16
    for i, f in enumerate(("input_ids_in", "input_ids_out", "probs_in", "probs_out", "beams_probs_in",
                           "beams_probs_out", "last_index_in", "last_index_out", "top_logprob", "top_token",
                           "all_finished")):
        setattr(a, f, 0x200000 + 0x1000 * i)   # never dereferenced: every call below is refused first
    a.input_ids_stride = a.probs_stride = 16
    return a


def test_beam_step_validates_without_a_device():
    from specdec_amd import _lib
    step = lambda a: _lib.lib.sd_beam_step(C.byref(a), None)
    assert _lib.lib.sd_beam_step(None, None) == _lib.SD_ERR_INVALID
    assert step(_lib.sd_beam_args()) == _lib.SD_ERR_INVALID
    a = _valid_step()
    assert step(a) == _lib.SD_ERR_WORKSPACE                       # everything valid but the workspace
    need = _lib.lib.sd_beam_workspace_size(4, 4096, 3)
    assert need > 0
    a.workspace, a.workspace_bytes = 0x900000, need - 1
    assert step(a) == _lib.SD_ERR_WORKSPACE
    for field in ("logits", "input_ids_in", "probs_out", "beams_probs_in", "last_index_out", "top_logprob",
                  "top_token", "all_finished"):
        a = _valid_step()
        setattr(a, field, None)
        assert step(a) == _lib.SD_ERR_INVALID, field
    for beams, k in ((65, 1), (4, 65), (64, 17)):
        a = _valid_step()
        a.num_beams, a.top_k = beams, k
        assert step(a) == _lib.SD_ERR_UNSUPPORTED, (beams, k)
    a = _valid_step()
    a.vocab = a.stride_r = 2                                       # top_k > vocab: torch.topk raises
    assert step(a) == _lib.SD_ERR_INVALID
    a = _valid_step()
    a.mode, a.vocab, a.stride_r = _lib.SD_BEAM_PREFILL, 3, 3       # num_beams > vocab in the prefill
    assert step(a) == _lib.SD_ERR_INVALID
    assert _lib.lib.sd_beam_workspace_size(65, 4096, 3) == 0
    assert _lib.lib.sd_beam_workspace_size(4, 2, 3) == 0
    # the partials lie behind the 8 MiB counter block every sd_* workspace layout starts with
    assert _lib.lib.sd_beam_workspace_size(64, 128256, 16) >= (8 << 20) + 64 * 34 * 63 * 4
    assert _lib.lib.sd_beam_workspace_size(1, 1, 1) >= (8 << 20)


def test_beam_host_wrappers_raise_the_references_errors():
    """Argument errors surface before any device work: an out-of-range position as IndexError, a k
    beyond the vocabulary with torch.topk's RuntimeError."""
    import pytest
    from specdec_amd import ops
    assert ops.beam_length_penalty(1, 1.2, 5.0) == 1.0
    assert ops.beam_length_penalty(3, 1.2, 5.0) == C.c_float(((5.0 + 3) / 6.0) ** 1.2).value
    assert ops.beam_length_penalty(0, 1.2, -0.0) == 1.0             # lp == 0 divides by 1
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        ops._beam_check_k(5, 4)
    ops._beam_check_k(4, 4)
