"""The vocabulary-parallel verify's host code under AddressSanitizer: `make asan-vp` links
csrc/vocab_parallel.hip's host-instrumented object (-Xarch_host -fsanitize=address) into
tests/asan/vp_asan.cpp, a stand-alone program that drives the argument checks of sd_vp_stats,
sd_vp_decide and sd_vp_finish (null pointers, γ' > 32, shard >= num_shards, a slice outside the
vocabulary, an empty slice, STREAM noise, top-k / nucleus processors, a short workspace) and the three
size functions over many shapes; an ASan report aborts it.  It runs as a child process; nothing is
loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speculative-decoding_amd")
BIN = os.path.join(PKG, "build", "asan", "vp_asan")


def test_vocab_parallel_host_code_is_asan_clean():
    r = subprocess.run(["make", "-C", PKG, "-j4", "asan-vp"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr
    assert ", 0 failed" in r.stdout
