"""The sd_vp_keep_* records and arguments: the ctypes mirrors against the header as gcc lays it out,
the size functions, and the refusals that need no GPU (host checks come before any launch)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "specdec.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sd_vp_keep_stat), offsetof(sd_vp_keep_stat, mass1),
           sizeof(sd_vp_keep_bin), offsetof(sd_vp_keep_bin, val), sizeof(sd_vp_keep_args),
           offsetof(sd_vp_keep_args, hist_local), offsetof(sd_vp_keep_args, round));
    return 0;
}
"""


@pytest.fixture(scope="module")
def L():
    from specdec_amd import _lib
    return _lib


def test_ctypes_mirrors_match_the_header(L, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    got = [C.sizeof(L.sd_vp_keep_stat), L.sd_vp_keep_stat.mass1.offset, C.sizeof(L.sd_vp_keep_bin),
           L.sd_vp_keep_bin.val.offset, C.sizeof(L.sd_vp_keep_args), L.sd_vp_keep_args.hist_local.offset,
           L.sd_vp_keep_args.round.offset]
    assert got == want and want[0] == 5136 and want[2] == 2064


def test_sizes_and_rounds(L):
    lib = L.lib
    assert lib.sd_vp_keep_hist_bytes(3, 4) == 32 + 3 * 9 * 5136
    assert lib.sd_vp_keep_bins_bytes(3, 4) == 32 + 3 * 9 * 2064
    assert lib.sd_vp_keep_hist_bytes(0, 4) == 0 and lib.sd_vp_keep_bins_bytes(1, L.SD_MAX_GAMMA + 1) == 0
    assert lib.sd_vp_keep_workspace_size(2, 1, 300) > lib.sd_vp_workspace_size(2, 1, 300) + 2 * 3 * 65536 * 4
    assert [lib.sd_vp_keep_rounds(k) for k in range(6)] == [0, 0, 1, 2, 3, 0]


@pytest.mark.parametrize("kind,dtype,noise,top_k,want", [
    ("SD_PROC_MULTINOMIAL", "SD_BF16", "SD_NOISE_PHILOX", 0, "SD_ERR_UNSUPPORTED"),   # sd_vp_* serves it
    ("SD_PROC_NUCLEUS", "SD_F32", "SD_NOISE_PHILOX", 0, "SD_ERR_UNSUPPORTED"),
    ("SD_PROC_TOPK", "SD_F16", "SD_NOISE_STREAM", 5, "SD_ERR_UNSUPPORTED"),
    ("SD_PROC_TOPK", "SD_BF16", "SD_NOISE_PHILOX", 0, "SD_ERR_INVALID"),
])
def test_refusals_before_any_launch(L, kind, dtype, noise, top_k, want):
    k = L.sd_vp_keep_args()
    a = k.vp
    a.batch, a.gamma, a.vocab, a.vocab_local, a.num_shards, a.dtype = 1, 0, 64, 64, 1, getattr(L, dtype)
    buf = (C.c_char * 64)()
    a.target_rows[0] = C.addressof(buf)
    a.proc = L.sd_processor(getattr(L, kind), 1.0, top_k, 0.9)
    a.noise.mode = getattr(L, noise)
    k.hist_local = C.addressof(buf)
    assert L.lib.sd_vp_keep_hist(C.byref(k), None) == getattr(L, want)
    assert L.lib.sd_vp_keep_finish(None, None) == L.SD_ERR_INVALID


def test_fake_ops_give_the_block_shapes(L):
    import torch
    import specdec_amd.torch_ops  # noqa: F401  (registers torch.ops.specdec.*)
    op, B, g = torch.ops.specdec, 5, 4
    t, d = torch.empty(B, g + 1, 100, dtype=torch.bfloat16, device="meta"), torch.empty(B, g, 100, dtype=torch.bfloat16, device="meta")
    tok, stops = torch.empty(B, g, dtype=torch.long, device="meta"), torch.empty(0, dtype=torch.long, device="meta")
    tail = (0, 2, 0, 200, L.SD_PROC_NUCLEUS, 1.0, 0, 0.9)
    hist = op.vp_keep_hist(t, d, tok, *tail)
    assert hist.shape == (L.lib.sd_vp_keep_hist_bytes(B, g),) and hist.dtype == torch.uint8
    hist_all = torch.empty(2, hist.shape[0], dtype=torch.uint8, device="meta")
    bins = op.vp_keep_refine(t, d, tok, hist_all, [], *tail)
    assert bins.shape == (L.lib.sd_vp_keep_bins_bytes(B, g),)
    bins_all = [torch.empty(2, bins.shape[0], dtype=torch.uint8, device="meta")] * 2
    cand = op.vp_keep_decide(t, d, tok, stops, hist_all, bins_all, *tail, False, 1, 0, 0)
    assert cand.shape == (L.lib.sd_vp_cand_bytes(B),)
    out = op.vp_keep_finish(torch.empty(2, cand.shape[0], dtype=torch.uint8, device="meta"), g, 0, 2, 0, 100, 200,
                            L.SD_PROC_NUCLEUS, 0, 0.9, 1, 0, 0)
    assert [tuple(o.shape) for o in out] == [(B,)] * 8 and out[1].dtype == torch.long
