"""The block-id fused verify's id split (csrc/sd_index.h): block id -> (sequence, slot, chunk), decider or
(sequence, sampler) by multiplying with host-computed reciprocals, against the `/` and `%` it replaced.

The header compiles for host and device; here the host compiler builds it into a small program that walks
every block id of every launch with B in {8, 9, 16, 24, 32, 40, 63}, 1..17 target slots, 1..64 spans a
row, 1..63 samplers a sequence and both placements where B % 8 == 0.  A launch's ids are the spans and
deciders [0, B per_seq) and then the samplers [B per_seq, B (per_seq + n_samp)); the split of a sampler id
does not depend on n_samp, so the ids of the launch with 63 samplers contain those of every launch with
fewer, and one walk per (B, slots, spans, placement) covers all of them.  It also walks the largest grids
the block-id layout can launch: the spans and deciders fill at most half of a residency of 256 x 8
workgroups, a sequence has at most 512 samplers (1024 sampling chunks, two each), and sd_fused_index_ok,
the launcher's range check, must admit them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speculative-decoding_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdint.h>
#include "sd_index.h"

static long long bad = 0, seen = 0;

/* the divisions the kernel ran before (stats_body, affine_split) */
static void check(int B, int nt, int nc, int xa, int ns) {
  const sd_fused_index x = sd_fused_index_make(B, nt, nc, xa);
  const int n_span = nt * nc, per_seq = n_span + 1;
  const long long total = (long long)B * (per_seq + ns);
  if (!sd_fused_index_ok(B, nt, nc, ns)) { ++bad; printf("range %d %d %d %d\n", B, nt, nc, ns); return; }
  for (long long id = 0; id < total; ++id) {
    int b, s = 0, chunk = 0, samp = -1, decider = 0;
    if (id >= (long long)B * per_seq) {
      const int t = (int)(id - (long long)B * per_seq);
      b = t % B;
      samp = t / B;
    } else {
      int item;
      if (xa) { const int w = (int)id & 7, k = (int)id >> 3; b = (k / per_seq) * 8 + w; item = k % per_seq; }
      else { b = (int)id / per_seq; item = (int)id - b * per_seq; }
      decider = item == n_span;
      s = item < n_span ? item / nc : 0;
      chunk = item < n_span ? item % nc : 0;
    }
    const sd_fused_item it = sd_fused_split(x, (uint32_t)id);
    ++seen;
    if (it.b != b || it.slot != s || it.chunk != chunk || it.samp != samp || it.decider != decider) {
      if (++bad < 10) printf("B=%d nt=%d nc=%d xa=%d id=%lld: (%d %d %d %d %d) want (%d %d %d %d %d)\n", B, nt, nc, xa, id,
                             it.b, it.slot, it.chunk, it.samp, it.decider, b, s, chunk, samp, decider);
    }
  }
}

int main(void) {
  static const int Bs[] = {8, 9, 16, 24, 32, 40, 63};
  for (unsigned i = 0; i < sizeof Bs / sizeof *Bs; ++i)
    for (int nt = 1; nt <= 17; ++nt)
      for (int nc = 1; nc <= 64; ++nc)
        for (int xa = 0; xa <= (Bs[i] % 8 == 0); ++xa) check(Bs[i], nt, nc, xa, 63);
  /* the largest grids: B per_seq <= 1024 spans and deciders, 512 samplers a sequence */
  check(512, 1, 1, 1, 512);
  check(512, 1, 1, 0, 512);
  check(341, 1, 2, 0, 512);
  check(8, 1, 64, 1, 512);    /* per_seq 65, head 520 */
  check(8, 2, 63, 1, 512);    /* per_seq 127, head 1016 */
  check(1, 16, 63, 0, 512);   /* per_seq 1009 */
  check(1, 17, 60, 0, 512);   /* per_seq 1021 */
  /* d = 1 and the range's edge for sd_div itself */
  for (uint32_t n = 0; n < 70000u; ++n) if (sd_div(n, sd_div_magic(1u)) != n) ++bad;
  for (uint32_t d = 1; d <= 4096u; ++d) {
    const uint32_t m = sd_div_magic(d), top = (uint32_t)(((1ull << 31) - 1u) / d);
    for (uint32_t n = top > 3000u ? top - 3000u : 0u; n <= top; ++n) { ++seen; if (sd_div(n, m) != n / d) ++bad; }
  }
  printf("seen %lld bad %lld\n", seen, bad);
  return bad != 0;
}
"""


def run(compiler, std, tmp_path):
    src = tmp_path / ("ix.c" if compiler == "gcc" else "ix.cpp")
    exe = tmp_path / ("ix_" + compiler.replace("+", "p"))
    src.write_text(PROGRAM)
    subprocess.check_call([compiler, std, "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert last[0] == "seen" and int(last[1]) > 100_000_000 and int(last[3]) == 0, res.stdout[-2000:]


def test_split_equals_division_for_every_block_id_c(tmp_path):
    run("gcc", "-std=c11", tmp_path)


def test_header_compiles_as_cxx_and_agrees(tmp_path):
    run("g++", "-std=c++17", tmp_path)
