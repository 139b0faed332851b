"""The dynamic draft trees' host code under AddressSanitizer: `make asan-tree-dynamic` links the
library's host-instrumented objects (-Xarch_host -fsanitize=address) into tests/asan/tree_dynamic_asan.cpp,
a stand-alone program that drives the argument checks of sd_tree_grow, sd_tree_select and
sd_verify_tree_dynamic (null pointers, W = 0 or 9, c > V, a pool above 2048, N > pool, max_depth 0 or 33,
STREAM noise, a short workspace) and their workspace-size functions over many shapes; an ASan report
aborts it.  It runs as a child process; nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speculative-decoding_amd")
BIN = os.path.join(PKG, "build", "asan", "tree_dynamic_asan")


def test_tree_dynamic_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-tree-dynamic"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
