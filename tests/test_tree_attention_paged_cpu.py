"""CPU checks of the paged-cache entries' host side (sd_tree_attention_paged, sd_kv_store_paged, sd_kv_compact_paged):
the ctypes mirrors of their argument structs have the C layout, and the argument checks run clean under
AddressSanitizer in a stand-alone program (tests/asan/tree_attn_paged_asan.cpp, linked by `make asan-tree-attn-paged`
with the host-instrumented objects of the three units) that hands every call fake device pointers.  The program runs
as a child process; nothing is loaded into this interpreter under a sanitizer."""
import os
import subprocess

import pytest

from test_tree_attention_fp8_cpu import PKG
from test_tree_attention_fp8_cpu import test_ctypes_layout_matches_the_header as _probe_layout

BIN = os.path.join(PKG, "build", "asan", "tree_attn_paged_asan")


@pytest.mark.parametrize("name", ["sd_tree_attention_paged_args", "sd_kv_store_paged_args", "sd_kv_compact_paged_args"])
def test_ctypes_layout_matches_the_header(name):
    """The FP8 structs' probe on the three new ones: every field, by name, at the C compiler's offset, and the same size."""
    _probe_layout(name)


def test_paged_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-tree-attn-paged"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stderr + r.stdout)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
