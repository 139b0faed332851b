"""Tree attention's host code under AddressSanitizer: `make asan-tree-attn` links the host-instrumented
object of csrc/tree_attention.hip (-Xarch_host -fsanitize=address) into tests/asan/tree_attn_asan.cpp, a
stand-alone program that drives the argument checks of sd_tree_attention (dtype, head_dim, rows, the GQA
group, kv_len, splits, strides, alignment, a short or missing workspace), the split rule and the workspace
arithmetic up to the largest shapes; an ASan report aborts it.  It runs as a child process; nothing is
loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speculative-decoding_amd")
BIN = os.path.join(PKG, "build", "asan", "tree_attn_asan")


def test_tree_attention_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-tree-attn"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
