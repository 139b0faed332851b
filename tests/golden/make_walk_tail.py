"""Writes tests/golden/walk_tail.json: what the library returns for the calls of
tests/test_gpu_walk_tail_golden.py (every integer output, resample_mass by its bit pattern, and the stop
lists derived from the accepted tokens).  Run it on a GPU with the library of the commit BEFORE the walks'
tails were shared (SPECDEC_LIB=<that build>.so, a file beside libspecdec.so): the test then holds the
shared tail to those outputs bit for bit.

    SPECDEC_LIB=libspecdec_parent.so python tests/golden/make_walk_tail.py [out.json]

The script makes every call twice and refuses to write a fixture if the two runs differ anywhere: a case
that is not bit-stable on the parent itself does not belong in the list.  (None had to be dropped.)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "speculative-decoding_amd"), os.path.join(ROOT, "tests"), ROOT]
import test_gpu_walk_tail_golden as t  # noqa: E402

sd = t.lib()
first = t.run_all(sd)
again = t.run_all(sd, first)
unstable = [c for c in first if first[c] != again[c]]
if unstable:
    sys.exit(f"not bit-stable across two runs: {unstable}")
hits = t.stop_hits(first)
assert all(hits[p] for p in t.PATHS), hits
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "walk_tail.json")
with open(out, "w") as f:
    json.dump(t.stored(first), f, separators=(",", ":"), sort_keys=True)
    f.write("\n")
n_seq = sum(len(e[k]["n_accepted"]) for e in first.values() for k in ("out", "out_stops") if k in e)
print(f"{len(first)} calls, {n_seq} sequences, stop hits {({p: len(v) for p, v in hits.items()})} -> {out}")
