"""Host-side proof that the inputs of tests/test_gpu_row_edges.py can do their job (no GPU, no library):
the oracle is finite on every one of them, masked rows keep a finite entry, the poison lies outside
every row and next to the first one, the recorded Philox seeds give walks with no close call and with
both accepting and rejecting rows, the reference raises on none of the verify inputs, a nucleus cut
at top_p = 1 drops at most the mass tolerance in either oracle, and the T = 0.05 deviation of the
torch-arithmetic oracle from the exact one is the recorded one."""
import dataclasses
import math

import pytest
import torch

import row_edges as re_
from oracle import specdec_ref as ref
from row_edges import DTYPES, F16, LAYOUTS, V_GRID, dt_name


def oracle_variants(proc):
    """tests/test_gpu_parity.py's oracle_variants (that module needs the library to import)."""
    out = [(proc, False), (proc, True)]
    if proc.kind in ("nucleus", "topknucleus"):
        st = dataclasses.replace(proc, stable_ties=True)
        out += [(st, False), (st, True)]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_name)
@pytest.mark.parametrize("V", V_GRID)
def test_oracle_is_finite_on_every_input(V, dtype):
    for mask in re_.MASKS:
        for what in ("probs", "sample"):
            x = re_.logits((4, V), dtype, re_.seed_of(what, V, mask), mask)
            finite = torch.isfinite(x.float())
            assert bool(finite.any(-1).all())                   # a masked row keeps a finite entry
            assert not bool(torch.isnan(x.float()).any()) and not bool((x.float() == math.inf).any())
            n_masked = {"none": 0, "half": V // 2, "most": V - min(V, 2 if V > 2 else 1)}[mask]
            assert (~finite).sum(-1).tolist() == [n_masked] * 4
            for kind, proc in re_.KINDS.items():
                for pv, exact in oracle_variants(proc):
                    if dtype == F16 and proc.kind in re_.KEEP_KINDS:
                        with pytest.raises(RuntimeError):       # the reference's -1e20 fill in fp16
                            ref.process(x, pv, exact)
                        assert kind not in re_.kinds_for(dtype)
                        continue
                    p = ref.process(x, pv, exact).float()
                    assert bool(torch.isfinite(p).all()) and bool((p >= 0).all()), (kind, mask)
                    assert bool((p[~finite] == 0).all())
                    assert bool(((p.double().sum(-1) - 1).abs() < 2e-2).all()), (kind, mask, p.sum(-1))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_name)
def test_poison_lies_outside_every_row(dtype, layout):
    item = torch.empty(0, dtype=dtype).element_size()
    vec = 16 // item
    for V in V_GRID:
        for lead in ((3,), (2, 5)):
            for poison in (math.inf, math.nan):
                x = re_.logits(lead + (V,), dtype, V)
                t = re_.place(x, layout, poison)
                buf = t.poisoned_buffer
                assert t.shape == x.shape and t.stride(-1) == 1 and torch.equal(t, x)
                R = math.prod(lead)
                margin, stride, n = re_.layout_geometry(R, V, dtype, layout)
                assert buf.numel() == n
                first = (t.data_ptr() - buf.data_ptr()) // item
                assert first == margin and margin * item >= 16
                inside = torch.zeros(n, dtype=torch.bool)
                for r in range(R):
                    inside[first + r * stride: first + r * stride + V] = True
                bad = torch.isnan(buf.float()) if poison != poison else buf.float() == math.inf
                assert torch.equal(bad, ~inside)                        # every element outside [0, V) of a row
                assert bool(bad[first - vec:first].all())               # the 16 bytes before the first row
                assert bool(bad[first + R * stride:][:vec].all()) and n - (first + R * stride) >= vec
                starts = [(first + r * stride) * item % 16 for r in range(R)]
                if layout == "padded":
                    assert starts == [0] * R and bool(bad[first + V: first + stride].all()) and stride - V >= vec
                if layout == "packed":
                    assert starts[0] == 0 and (all(s == 0 for s in starts) == (V * item % 16 == 0))
                if layout == "shifted":
                    assert starts[0] == item


def test_poison_is_half_inf_half_nan():
    kinds = [re_.poison_of(layout, V, dtype, mask) for layout in LAYOUTS for V in V_GRID for dtype in DTYPES
             for mask in re_.MASKS]
    n_inf = sum(1 for p in kinds if p == math.inf)
    assert 0.3 * len(kinds) <= n_inf <= 0.7 * len(kinds)


def test_one_ulp_helper():
    for dtype in DTYPES:
        w = torch.tensor([0.0, 0.25, 0.1, 1.0], dtype=dtype)
        up = torch.nextafter(w.float(), torch.tensor(2.0)).to(dtype) if dtype == torch.float32 else \
            (w.view(torch.int16) + 1).view(dtype)
        assert bool(re_.within_one_ulp(up, w).all()) and bool(re_.within_one_ulp(w, w).all())
        assert not bool(re_.within_one_ulp(w * 1.5, w)[1:].any())


def test_rank_close():
    assert not re_.rank_close(torch.tensor([1.0, 1.0, -math.inf, 2.0]))
    assert re_.rank_close(torch.tensor([3.5304579734802246, 3.530458688735962, 0.0]))
    assert not re_.rank_close(torch.randn(64).bfloat16() * 3)


@pytest.mark.parametrize("key", re_.philox_keys(), ids=lambda k: f"{k[0]}-B{k[1]}-g{k[2]}-V{k[3]}-{dt_name(k[4])}")
def test_philox_seeds(key):
    """The recorded seed: no row a close call, an accepting and a rejecting row; and the lowest such."""
    rule, B, g, V, dtype = key
    seed = re_.PHILOX_SEEDS[key]
    pc = re_.philox_case(*key)
    live = [r for r in pc.rows if r.active]
    assert not any(r.close for r in live)
    assert any(r.want > 0 for r in live) and any(r.rejected for r in live)
    assert re_.find_philox_seed(*key, limit=seed + 1) == seed
    assert pc.noise[1] == re_.PHILOX_NOISE[rule][1] + seed


# ---------------------------------------------------------------- STREAM verify inputs
def spec_oracles_run(B, gamma, V, dtype, proc, seed):
    """Every oracle variant of test_gpu_parity.py::check_spec runs on the case (the reference raises on
    a rejected draft whose residual is all zero)."""
    import test_gpu_parity as par        # its helpers need no library; its tests are marked gpu
    tl, dl, ids = par.draft_case(B, gamma, V, dtype, seed, proc)
    try:
        for _, pv, exact in par.oracle_variants(proc):
            par.run_spec_oracle(tl, dl, ids, pv, torch.Generator().manual_seed(1000 + seed), [], False, exact)
    except RuntimeError:
        return False
    return True


@pytest.mark.parametrize("dtype", re_.STREAM_DTYPES + (F16,), ids=dt_name)
@pytest.mark.parametrize("V", V_GRID)
def test_stream_verify_inputs_run_on_the_oracle(V, dtype):
    if dtype == F16:
        if V < 64:
            assert spec_oracles_run(3, 4, V, F16, re_.KINDS["multi_t1"], re_.seed_of("spec16", V))
        return
    for B, gamma in re_.STREAM_BG:
        for kind in re_.STREAM_KINDS:
            bump = re_.STREAM_BUMPS.get((V, dtype, B, gamma, kind), 0)
            for lower in range(bump):       # the seeds passed over do raise
                assert not spec_oracles_run(B, gamma, V, dtype, re_.KINDS[kind], re_.stream_seed(V, dtype, B, gamma, kind, lower))
            assert spec_oracles_run(B, gamma, V, dtype, re_.KINDS[kind], re_.stream_seed(V, dtype, B, gamma, kind))
    assert all(k[0] in V_GRID and k[1] in re_.STREAM_DTYPES and k[2:4] in re_.STREAM_BG and k[4] in re_.STREAM_KINDS
               for k in re_.STREAM_BUMPS)


# ---------------------------------------------------------------- processor extremes
@pytest.mark.parametrize("dtype", re_.EXTREME_DTYPES, ids=dt_name)
@pytest.mark.parametrize("V", re_.EXTREME_V)
def test_extreme_inputs(V, dtype):
    for mask in re_.EXTREME_MASKS:
        x = re_.extreme_logits(4, V, dtype, mask)
        finite = torch.isfinite(x.float())
        assert bool(finite.any(-1).all()) and not bool(torch.isnan(x.float()).any())
        if mask == "tied":
            assert bool(((x == x.max(-1, keepdim=True).values).sum(-1) >= 2).all())
        for name, proc in re_.extreme_procs(V).items():
            for pv, exact in oracle_variants(proc):
                p = ref.process(x, pv, exact).float()
                assert bool(torch.isfinite(p).all()) and bool((p >= 0).all()), (name, mask)
                assert bool((p[~finite] == 0).all())
                if name == "nucleus1" and pv.stable_ties:
                    # the cut at top_p = 1 is decided by rounding alone; what it drops is negligible
                    assert float(re_.dropped_mass(x, p > 0).max()) <= 1e-5, (mask, exact)
                if name in ("nucleus0", "nucleus1e-06") and pv.stable_ties:
                    assert (p > 0).sum(-1).tolist() == [1] * 4
                    assert torch.equal(p.argmax(-1), x.float().argmax(-1))
                if name == "topk1":
                    assert torch.equal(p > 0, x == x.max(-1, keepdim=True).values)
    for name, proc in re_.extreme_procs(V).items():
        assert spec_oracles_run(1, 4, V, dtype, proc, re_.extreme_spec_seed(V, name)), name


def test_cold_deviation_is_the_recorded_one():
    assert re_.cold_deviation() == pytest.approx(re_.COLD_DEVIATION_F32, rel=1e-3)
    assert re_.COLD_RTOL_F32 == max(2e-6, 4 * re_.COLD_DEVIATION_F32)
