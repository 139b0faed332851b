"""Writes tests/golden/draw_onepass.json: what the library returns for the draws of
tests/test_gpu_draw_onepass.py (tokens, token_prob, row statistics and row status, the floats by their bit
patterns).  Run it on a GPU with the library of the commit BEFORE k_draw_lean's tail took its pass count as
a parameter (SPECDEC_LIB=<that build>.so, a file beside libspecdec.so), whose tail runs two lane passes for
every row: the test then holds the one-pass tail to those outputs bit for bit.

    SPECDEC_LIB=libspecdec_parent.so python tests/golden/make_draw_onepass.py [out.json]

The script makes every call twice and refuses to write a fixture if the two runs differ anywhere."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "speculative-decoding_amd"), os.path.join(ROOT, "tests"), ROOT]
import test_gpu_draw_onepass as t  # noqa: E402

sd = t.lib()
first = t.run_all(sd)
again = t.run_all(sd)
unstable = [c for c in first if first[c] != again[c]]
if unstable:
    sys.exit(f"not bit-stable across two runs: {unstable}")
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "draw_onepass.json")
with open(out, "w") as f:
    json.dump(first, f, separators=(",", ":"), sort_keys=True)
    f.write("\n")
print(f"{len(first)} cases, {sum(len(v) for v in first.values())} calls -> {out}")
