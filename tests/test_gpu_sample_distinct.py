"""sd_sample_distinct (csrc/sample_distinct.hip) against the fp64 Gumbel top-k on the same Philox words: tokens rank
for rank, keys within the key tolerance (tests/test_tree_swor_cpu.py: no rank here is a close call)."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tree_swor_ref as sw
from oracle import specdec_ref as ref

DEV = "cuda"
SEED, OFFSET, ROW_BASE, ROWS = 0xD157C7, 3, 11, 3
PROCS = {"multinomial": ref.Processor("multinomial", 1.0), "topk3": ref.Processor("topk", 1.0, top_k=3),
         "nucleus0.9": ref.Processor("nucleus", 1.0, top_p=0.9, stable_ties=True)}
# V x k x dtype x processor; packed | padded rows alternate along the (dtype, processor) and the (V, k) index
CASES = [c + (("packed", "padded")[(i + i // 6) % 2],) for i, c in enumerate(itertools.product(
    [1, 7, 2048, 2049, 4101], [1, 3, 8], [torch.bfloat16, torch.float32], list(PROCS)))]


@functools.lru_cache(maxsize=None)
def host(V, k, dtype, name, layout):
    gen = torch.Generator().manual_seed(V * 131 + k)
    logits = (torch.randn(ROWS, V, generator=gen) * 3).to(dtype)
    W = ref.process(logits, PROCS[name], exact=True).double().numpy()
    draws = [sw.gumbel_topk(W[r], k, SEED, OFFSET, ROW_BASE + r) for r in range(ROWS)]
    return SimpleNamespace(logits=logits, tokens=np.stack([d[0] for d in draws]), keys=np.stack([d[1] for d in draws]),
                           close=sum(len(d[2]) for d in draws))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"V{c[0]}-k{c[1]}-{str(c[2]).split('.')[-1]}-{c[3]}-{c[4]}")
def test_draws_equal_the_host_model(case):
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    V, k, dtype, name, layout = case
    h = host(*case)
    logits = h.logits.to(DEV)
    if layout == "padded":                             # rows 16-byte misaligned inside NaN
        logits = torch.full((ROWS, V + 13), float("nan"), dtype=dtype, device=DEV)[:, 5:5 + V].copy_(logits)
    p, status = PROCS[name], torch.zeros(1, dtype=torch.int32, device=DEV)
    tok, keys = ops.sample_distinct(logits, k, ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p),
                                    PhiloxNoise(seed=SEED, offset=OFFSET), status_or=status, row_base=ROW_BASE)
    assert _lib.last_sample_path() == _lib.SD_PATH_SAMPLE_DISTINCT
    tok, keys = tok.cpu().numpy(), keys.cpu().numpy().astype(np.float64)
    drawn = h.tokens >= 0
    err = float(np.abs(keys[drawn] - h.keys[drawn]).max())
    print(f"[distinct] {case} key_err={err:.3g} tol={sw.KEY_TOL:.3g} minus_ones={int((~drawn).sum())}")
    assert int(status.item()) == 0 and np.array_equal(tok, h.tokens), (tok, h.tokens)
    assert np.all(np.isneginf(keys[~drawn])) and err <= sw.KEY_TOL
    assert (name, k) != ("topk3", 8) or V < 7 or (~drawn).sum() == 5 * ROWS   # three tokens keep weight: five -1 per row
