"""Writes tests/golden/arg_preload_draw.json: what the library returns for the lean-draw calls of
tests/test_gpu_arg_preload.py (tokens, the row statistics' bit patterns, the status).  Run it on a GPU
with the library of the commit BEFORE the kernel-argument change (SPECDEC_LIB=<that build>.so, a file
beside libspecdec.so): the test then holds the new argument path to those outputs bit for bit.

    SPECDEC_LIB=libspecdec_parent.so python tests/golden/make_arg_preload.py [out.json]"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "speculative-decoding_amd"), os.path.join(ROOT, "tests"), ROOT]
import test_gpu_arg_preload as t  # noqa: E402

out = {}
for case in t.DRAW_CASES:
    tok, stats, st, _ = t.run_draw(case)
    out[t.case_id(case)] = {"tokens": tok.tolist(), "stats_bits": stats.view(torch.int32).flatten().tolist(),
                            "status": st.tolist()}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "arg_preload_draw.json")
with open(path, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print(f"{len(out)} cases -> {path}")
