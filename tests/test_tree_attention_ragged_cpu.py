"""CPU checks of sd_tree_attention_ragged's host side: the ctypes mirror of its argument struct has the C
layout, and the argument checks, the chunk rule and the workspace arithmetic run clean under
AddressSanitizer in a stand-alone program (tests/asan/tree_attn_ragged_asan.cpp, linked by
`make asan-tree-attn-ragged` with the host-instrumented object of csrc/tree_attention.hip) that hands
every call fake device pointers.  The program runs as a child process; nothing is loaded into this
interpreter under a sanitizer."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speculative-decoding_amd")
BIN = os.path.join(PKG, "build", "asan", "tree_attn_ragged_asan")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "specdec.h"
#define F(f) printf(#f " %zu\n", offsetof(sd_tree_attention_ragged_args, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(sd_tree_attention_ragged_args));
  F(batch) F(heads_q) F(heads_kv) F(rows) F(head_dim) F(dtype) F(kv_cap) F(kv_alloc) F(chunk_tiles) F(scale)
  F(q) F(q_stride_b) F(q_stride_h) F(q_stride_r) F(k) F(v) F(k_stride_b) F(k_stride_h) F(k_stride_pos)
  F(v_stride_b) F(v_stride_h) F(v_stride_pos) F(out) F(out_stride_b) F(out_stride_r) F(out_stride_h)
  F(kv_limit) F(win_bits) F(kv_len_dev) F(kv_len_add) F(win_base_dev) F(win_base_add) F(status_or)
  F(workspace) F(workspace_bytes)
  return 0;
}
"""


def test_ctypes_layout_of_the_ragged_args_matches_the_header():
    from specdec_amd import _lib
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(PROBE)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    cls = _lib.sd_tree_attention_ragged_args
    assert int(got.pop("sizeof")) == C.sizeof(cls)
    assert list(got) == [name for name, _ in cls._fields_]
    for name, offset in got.items():
        assert getattr(cls, name).offset == int(offset), name


def test_ragged_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-tree-attn-ragged"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
