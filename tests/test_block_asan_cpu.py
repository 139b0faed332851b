"""The block verify's host code under AddressSanitizer: `make asan-block` links the library's
host-instrumented objects (-Xarch_host -fsanitize=address) into tests/asan/block_asan.cpp, a
stand-alone program that drives sd_verify_block's argument checks (null pointers, γ' = 0 or 33, bad
enums, mixed dtypes, STREAM noise, a short workspace) and sd_verify_block_workspace_size over many
shapes; an ASan report aborts it.  It runs as a child process; nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speculative-decoding_amd")
BIN = os.path.join(PKG, "build", "asan", "block_asan")


def test_block_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-block"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
