"""The kernel-argument layouts of k_draw_lean and of the block-id k_verify_fused (leading scalar
parameters, preloaded into SGPRs on gfx950): only the point where a kernel learns its
arguments moved, so every output keeps its bits.

Lean draw.  V = 8 (one vector), 2048 (exactly one span), 2056 (a second span of one vector) and 4104 (a
ragged third span), 1 and 3 rows, bf16 / fp16, multinomial / greedy, contiguous rows and rows padded to a
stride of V + 8.  Checked three ways:
  * bit for bit against what the parent commit's library returned for the same calls
    (tests/golden/arg_preload_draw.json, written by tests/golden/make_arg_preload.py): tokens, the
    (max, sum) row statistics and the status;
  * against the general path — the same values in rows that are not 16-byte aligned, which k_draw_lean
    does not take: equal status, equal greedy tokens (both are the exact argmax rule) and row statistics
    that agree to 2e-6 relative.  The multinomial TOKENS of the two kernels differ by design (k_draw picks
    the span by an fp64 CDF scan, k_draw_lean by a Gumbel race on other Philox words), so they are not
    compared with each other here: which token each kernel must return is held, row by row, to the fp64
    host model of both rules in tests/test_gpu_draw_exact.py (tests/draw_ref.py), and the recorded parent
    outputs above only pin the bits;
  * the oracle check of tests/test_gpu_draw.py: exp(y - M) / S is the fp64 softmax to 2e-6 relative on
    the largest probabilities (the greedy token: the first index of the row's top rounded probability).

Fused verify.  B = 8 (XCD-affine placement) and 9 (plain), gamma 1 and 4, V = 2056, bf16 / fp16, the
target rows given as views of a [B, T, V] tensor, as views of a [T, B, V] tensor, as separately allocated
tensors in shuffled address order (the table path) and with every slot one tensor (spacing 0), each with
SD_OPT_ARG_FAST on and off: all outputs, the engine state and the row counts are equal bit for bit
across the runs and equal the two-launch path's.  A hipGraph of two steps replayed three times returns
the eager steps' outputs (preloaded arguments survive replay)."""
import contextlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arg_preload_draw.json")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
DRAW_CASES = [(V, B, dt, kind, layout) for V in (8, 2048, 2056, 4104) for B in (1, 3) for dt in DTYPES
              for kind in ("multinomial", "greedy") for layout in ("contiguous", "padded")]


def case_id(c):
    return "V{}-B{}-{}-{}-{}".format(*c)


def draw_values(V, B, dt):
    g = torch.Generator().manual_seed(1000 * V + 10 * B + (1 if dt == "fp16" else 0))
    return (torch.randn(B, V, generator=g) * 3).to(DTYPES[dt])


def place(x, layout):
    """x on the device: contiguous, rows at a stride of V + 8 elements, or ("general") contiguous rows
    that start 2 bytes past a 16-byte boundary, which k_draw_lean does not take."""
    B, V = x.shape
    if layout == "contiguous":
        return x.to(DEV)
    if layout == "padded":
        buf = torch.zeros(B, V + 8, dtype=x.dtype, device=DEV)
        buf[:, :V] = x.to(DEV)
        return buf[:, :V]
    buf = torch.zeros(B * V + 8, dtype=x.dtype, device=DEV)
    view = buf[1:1 + B * V].view(B, V)
    view.copy_(x.to(DEV))
    assert view.data_ptr() % 16 == 2
    return view


def run_draw(case, layout=None):
    """One sd_sample call of the case: (tokens, stats as int32 bit patterns, status), on the host."""
    from specdec_amd import PhiloxNoise, _lib, ops
    V, B, dt, kind, lay = case
    rows = place(draw_values(V, B, dt), layout or lay)
    stats = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    tok, _, st = ops.sample_rows(rows, ops.ProcSpec(kind, 1.0), PhiloxNoise(seed=77 + V, offset=3), row_stats_out=stats)
    torch.cuda.synchronize()
    return tok.cpu(), stats.cpu(), st.cpu(), _lib.last_sample_path()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", DRAW_CASES, ids=case_id)
def test_lean_draw_keeps_its_bits(case, golden):
    from specdec_amd import _lib
    V, B, dt, kind, _ = case
    tok, stats, st, path = run_draw(case)
    assert path == (_lib.SD_PATH_SAMPLE_GREEDY_LEAN if kind == "greedy" else _lib.SD_PATH_SAMPLE_DRAW_LEAN), _lib.PATH_NAMES.get(path)
    # the parent commit's outputs for this call
    want = golden[case_id(case)]
    assert tok.tolist() == want["tokens"]
    assert stats.view(torch.int32).flatten().tolist() == want["stats_bits"]
    assert st.tolist() == want["status"]
    # the general path on the same values
    gtok, gstats, gst, gpath = run_draw(case, "general")
    assert gpath not in (_lib.SD_PATH_SAMPLE_GREEDY_LEAN, _lib.SD_PATH_SAMPLE_DRAW_LEAN), _lib.PATH_NAMES.get(gpath)
    assert torch.equal(st, gst)
    assert st.tolist() == [_lib.SD_ROW_DONE] * B
    x = draw_values(V, B, dt).double()
    exact = torch.softmax(x, dim=-1)
    # (greedy: the general path is the three-launch one, compared on its tokens and status only)
    for name, s in (("lean", stats), ("general", gstats))[:1 if kind == "greedy" else 2]:
        p = torch.exp(x - s[:, 0:1].double()) / s[:, 1:2].double()
        top = exact >= exact.max(dim=-1, keepdim=True).values * 1e-3
        rel = float(((p - exact).abs() / exact)[top].max())
        print(f"[arg-preload] {case_id(case)} {name}: softmax rel err {rel:.3g}")
        assert rel < 2e-6, (name, rel)
    if kind == "greedy":
        assert torch.equal(tok, gtok)
        # the oracle of tests/test_gpu_greedy.py: torch-CPU arithmetic (the reference) or exact softmax
        from test_gpu_greedy import oracle_tokens
        ora = oracle_tokens(draw_values(V, B, dt))
        assert all(int(tok[b]) in (int(ora[0][b]), int(ora[1][b])) for b in range(B)), (tok, ora)
    else:
        assert torch.equal(stats[:, 0], gstats[:, 0])   # the row maximum is exact on both paths
        assert float(((stats[:, 1] - gstats[:, 1]).abs() / gstats[:, 1]).max()) < 2e-6
        assert ((tok >= 0) & (tok < V)).all()


# ---------------------------------------------------------------- fused verify
def option(name, value):
    from specdec_amd import _lib
    return _lib.option(getattr(_lib, name), value)


def verify_inputs(B, g, V, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, g + 1, V, generator=gen) * 3).to(DTYPES[dt])
    dl = (tl[:, :g].float() + torch.randn(B, g, V, generator=gen)).to(DTYPES[dt])
    return tl.to(DEV), dl.to(DEV)


def target_rows(tl, way):
    """The g + 1 target rows [B, V] of tl [B, g + 1, V], laid out in one of the four ways."""
    B, T, V = tl.shape
    if way == "bgv":
        return [tl[:, t] for t in range(T)]
    if way == "gbv":
        tt = tl.transpose(0, 1).contiguous()
        return [tt[t] for t in range(T)]
    if way == "separate":
        # separately allocated, handed over so that the addresses are neither ascending nor evenly spaced
        pool = [torch.empty(B, V, dtype=tl.dtype, device=DEV) for _ in range(T + 2)]
        pool.sort(key=lambda t: t.data_ptr())
        order = [pool[i] for i in ([1, 0] + list(range(3, T + 2)) + [2])][:T] if T > 1 else [pool[1]]
        if T > 2:
            d = [order[i + 1].data_ptr() - order[i].data_ptr() for i in range(T - 1)]
            assert len(set(d)) > 1 or d[0] < 0
        else:
            assert T == 1 or order[1].data_ptr() < order[0].data_ptr()
        for t in range(T):
            order[t].copy_(tl[:, t])
        return order
    assert way == "alias"
    one = tl[:, 0].contiguous()
    return [one] * T


def run_verify(trows, dl, rule, seed):
    from specdec_amd import PhiloxNoise, _lib, ops
    B, g = dl.shape[0], dl.shape[1]
    spec = ops.ProcSpec("multinomial", 1.0)
    noise = PhiloxNoise(seed=seed)
    draft = torch.zeros(B, g, dtype=torch.long, device=DEV)
    stats = torch.empty(g, B, 2, device=DEV)
    for d in range(g):
        ops.sample_rows(dl[:, d], spec, noise, tokens_out=draft[:, d], row_stats_out=stats[d])
    extra, state = {}, None
    n_t = g
    if rule == "engine":
        state = dict(generated=torch.zeros(B, 3 * g, dtype=torch.long, device=DEV), step=g,
                     finished=torch.zeros(B, dtype=torch.uint8, device=DEV), accepted=torch.zeros(B, dtype=torch.long, device=DEV))
        extra = dict(engine_state=state, active=(torch.arange(B, device=DEV) % 5 != 3).to(torch.uint8))
    else:
        n_t = g + 1
    counts = torch.zeros(B, 2, dtype=torch.long, device=DEV)
    out = ops.verify(trows[:n_t], [dl[:, d] for d in range(g)], draft, _lib.SD_RULE_SPEC if rule == "spec" else _lib.SD_RULE_ENGINE,
                     spec, spec, noise, torch.tensor([int(draft[0, 0])], device=DEV), draft_row_stats=stats,
                     row_counts=counts, **extra)
    torch.cuda.synchronize()
    res = {k: getattr(out, k).cpu() for k in ("n_accepted", "next_token", "row_status", "resample_mass")}
    res["counts"] = counts.cpu()
    if state is not None:
        res.update({k: v.cpu() for k, v in state.items() if torch.is_tensor(v)})
    return res, _lib.last_verify_path()


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].nan_to_num().view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                    b[k].nan_to_num().view(torch.int32) if b[k].dtype == torch.float32 else b[k])
                                        for k in a)


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("B", [8, 9])
def test_fused_verify_row_layouts(B, g, dt, rule):
    from specdec_amd import _lib
    V = 2056
    seed = 100 * B + 10 * g + (1 if dt == "fp16" else 0)
    tl, dl = verify_inputs(B, g, V, dt, seed)
    ref = {}
    for way in ("bgv", "gbv", "separate", "alias"):
        trows = target_rows(tl, way)
        with option("SD_OPT_FUSED_VERIFY", 0), option("SD_OPT_LEAN_VERIFY", 0):
            two, path = run_verify(trows, dl, rule, seed)
        assert path == _lib.SD_PATH_VERIFY_TWO_LAUNCH, _lib.PATH_NAMES.get(path)
        for fast in (1, 0):
            with option("SD_OPT_ARG_FAST", fast), option("SD_OPT_LEAN_VERIFY", 0):
                got, path = run_verify(trows, dl, rule, seed)
            assert path == _lib.SD_PATH_VERIFY_FUSED, _lib.PATH_NAMES.get(path)
            assert same(got, two), (way, fast, got, two)
        active = (torch.arange(B) % 5 != 3) if rule == "engine" else torch.ones(B, dtype=torch.bool)
        assert (two["row_status"][active] & _lib.SD_ROW_DONE).all()
        assert not (two["row_status"] & _lib.SD_ROW_ERROR_MASK).any()
        # the same logits, however the rows are laid out
        if way != "alias":
            ref.setdefault("out", two)
            assert same(ref["out"], two), way


def test_arg_fast_option_defaults_on():
    from specdec_amd import _lib
    assert _lib.get_option(_lib.SD_OPT_ARG_FAST) == 1
    with _lib.option(_lib.SD_OPT_ARG_FAST, 0):
        assert _lib.get_option(_lib.SD_OPT_ARG_FAST) == 0
    assert _lib.get_option(_lib.SD_OPT_ARG_FAST) == 1


def test_graph_of_two_steps_replays_the_eager_outputs():
    from specdec_amd import PhiloxNoise, _lib, ops
    B, g, V = 8, 4, 2056
    tl, dl = verify_inputs(B, g, V, "bf16", 5)
    spec = ops.ProcSpec("multinomial", 1.0)
    draft = torch.zeros(2, B, g, dtype=torch.long, device=DEV)
    stats = torch.empty(2, g, B, 2, device=DEV)
    stop = torch.tensor([V - 1], device=DEV)

    def two_steps():
        noise = PhiloxNoise(seed=9)
        outs = []
        for s in range(2):
            for d in range(g):
                ops.sample_rows(dl[:, d], spec, noise, tokens_out=draft[s, :, d], row_stats_out=stats[s, d])
            o = ops.verify([tl[:, t] for t in range(g + 1)], [dl[:, d] for d in range(g)], draft[s], _lib.SD_RULE_SPEC, spec, spec,
                           noise, stop, draft_row_stats=stats[s])
            outs += [o.n_accepted, o.next_token, o.row_status]
        return outs

    with option("SD_OPT_LEAN_VERIFY", 0):
        eager = [t.clone() for t in two_steps()] + [draft.clone(), stats.clone()]
        assert _lib.last_verify_path() == _lib.SD_PATH_VERIFY_FUSED
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            two_steps()
            with torch.cuda.graph(graph, stream=stream):
                outs = two_steps()
        torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        draft.zero_()
        stats.zero_()
        for t in outs:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs + [draft, stats], eager):
            assert torch.equal(got, want)
