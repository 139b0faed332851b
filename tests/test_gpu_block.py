"""sd_verify_block on the GPU: one drafted chain per sequence verified jointly (block verification).

* every case of block_cases.grid() against the host model (tests/block_ref.py over the exact-arithmetic
  oracle and the numpy Philox), with and without the draws' hints: n, status, stop_index, the prune
  lengths and tokens_out exactly, weights and accept_prob within the bounds block_ref derives,
  resample_mass within the mass bound, the token by the widened-interval check.  A `close` sequence (a
  decision or a draw within the device's error bound; at most 5 % of the grid, tests/test_block_cpu.py)
  is skipped;
* γ' = 1, and any γ' whose ratios are all >= 1, against sd_verify(SD_RULE_SPEC);
* flagged rows, workspace reuse across entry points, sd_last_verify_path, graph capture;
* losslessness and the acceptance gain on the device, statistically.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import block_cases as bc
import block_ref as br
import multi_walk as mw
import multidraft_ref as mref
import row_edges as rowe
from test_gpu_perfmode import chi2_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7
INT_FIELDS = ("n_accepted", "prune_drafter", "prune_target", "stop_index", "row_status")


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def draw_hints(sd, dl, proc):
    """(stats [γ, B, 2], keeps [γ, B, 4] or None) of the drafter rows dl [B, γ, V] as sd_sample returns
    them with its draws; the drawn tokens are discarded — the tests choose the drafts."""
    B, g, V = dl.shape
    spec = spec_of(sd, proc)
    stats = torch.empty(g, B, 2, device=DEV)
    keeps = torch.empty(g, B, 4, dtype=torch.int32, device=DEV) if spec.keeps else None
    noise = sd.PhiloxNoise(seed=4242)
    for d in range(g):
        sd.ops.sample_rows(dl[:, d, :].contiguous(), spec, noise, row_stats_out=stats[d],
                           row_keep_out=keeps[d] if keeps is not None else None)
    return stats, keeps


def run_block(sd, tl, dl, tok, proc, seed, off, row_base=0, stops=(), hints=False, **kw):
    if hints:
        kw["draft_row_stats"], kw["draft_row_keep"] = draw_hints(sd, dl, proc)
    out = sd.ops.verify_block(tl, dl, tok, spec_of(sd, proc), sd.PhiloxNoise(seed=seed, offset=off),
                              stop_tokens=torch.tensor(list(stops), dtype=torch.long, device=DEV), row_base=row_base,
                              pad_token_id=PAD, **kw)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_BLOCK
    fields = sd.ops.BLOCK_FIELDS + ("weights", "accept_prob", "tokens_out")
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in fields})


def on_device(c):
    """The case's rows in its layout inside a poisoned buffer on the device."""
    poison = rowe.poison_of("block", c.B, c.gamma, c.V, c.layout)
    if c.layout == "packed":
        return c.tl.to(DEV), c.dl.to(DEV)
    return rowe.place(c.tl, c.layout, poison, DEV), rowe.place(c.dl, c.layout, poison, DEV)


def check_case(sd, c, got, rows):
    L, g = sd.lib, c.gamma
    skipped = 0
    for b, r in enumerate(rows):
        n, st, x = int(got.n_accepted[b]), int(got.row_status[b]), int(got.next_token[b])
        ints = (n, int(got.prune_drafter[b]), int(got.prune_target[b]), int(got.stop_index[b]))
        want = (r.n, r.prune_drafter, r.prune_target, r.stop_index)
        print(f"[block] b={b} got={ints} want={want} tokenwise_n={r.tokenwise_n} close={r.close} status=0x{st:x} x={x} "
              f"mass={float(got.resample_mass[b]):.6g}/{r.mass:.6g}")
        assert st & L.SD_ROW_DONE
        # the diagnostics hold whatever the decisions: they do not depend on the uniforms
        for t in range(g + 1):
            dev_w = float(got.weights[b, t])
            assert abs(dev_w - r.w[t]) <= br.weight_bound(t), (b, t, dev_w, r.w[t])
        for t in range(1, g + 1):
            dev_h = float(got.accept_prob[b, t - 1])
            print(f"[block-h] b={b} t={t} dev={dev_h:.9g} host={r.h[t]:.9g} lo={r.h_lo[t]:.9g} hi={r.h_hi[t]:.9g}")
            assert r.h_lo[t] <= dev_h <= r.h_hi[t], (b, t, dev_h, r.h[t], r.h_lo[t], r.h_hi[t])
        if r.close:
            skipped += 1
            continue
        assert not st & L.SD_ROW_ERROR_MASK
        assert ints == want, (b, ints, want)
        want_bit = {br.RESIDUAL: L.SD_ROW_RESIDUAL, br.BONUS: L.SD_ROW_BONUS, br.STOP: L.SD_ROW_STOP_IN_DRAFTS}
        assert st & (L.SD_ROW_RESIDUAL | L.SD_ROW_BONUS | L.SD_ROW_STOP_IN_DRAFTS) == want_bit[r.status], (b, hex(st))
        if r.n < g:
            tol = br.mass_bound(c.s_tol[b][r.n], r.n)
            print(f"[block-mass] b={b} n={r.n} dev={abs(float(got.resample_mass[b]) - r.mass):.3g} bound={tol:.3g}")
            assert abs(float(got.resample_mass[b]) - r.mass) <= tol + 2.0 ** -23 * r.mass
        else:
            assert np.isnan(float(got.resample_mass[b]))
        row = got.tokens_out[b].tolist()
        assert row[:n] == c.tok[b, :n].tolist()
        if r.status == br.STOP:
            assert x == -1 and row[n:] == [PAD] * (g + 1 - n)
            continue
        assert 0 <= x < c.V and row[n] == x and row[n + 1:] == [PAD] * (g - n)
        if c.proc.stochastic:
            assert r.weights[x] > 0, (b, x)
            used = mw.draw_excess(r, x, r.draw_slack)
            lo, hi = mref.draw_interval(r.weights, x)
            print(f"[block-draw] b={b} x={x} host_x={r.x} target={r.u * r.total:.9g} lo={lo:.9g} hi={hi:.9g} "
                  f"slack={r.draw_slack:.3g} used={used:.3g}")
            assert used <= 1.0, (b, x, r.x)
        else:
            assert r.weights[x] >= r.weights.max() * (1 - 1e-4), (b, x, r.x)
    assert skipped == sum(r.close for r in rows)


# ---------------------------------------------------------------- the grid against the host model
@pytest.mark.parametrize("hints", [False, True], ids=["stats-in-verify", "stats-from-draws"])
@pytest.mark.parametrize("case", bc.grid(), ids=bc.case_id)
def test_steps_equal_the_host_model(sd, case, hints):
    c = bc.case(*case)
    tl, dl = on_device(c)
    got = run_block(sd, tl, dl, c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, c.stops, hints=hints)
    check_case(sd, c, got, c.rows)


# ---------------------------------------------------------------- where the rule is sd_verify's
def _spec_verify(sd, c, tok, stops):
    tl, dl = c.tl.to(DEV), c.dl.to(DEV)
    spec = spec_of(sd, c.proc)
    g = c.gamma
    return sd.ops.verify([tl[:, t] for t in range(g + 1)], [dl[:, t] for t in range(g)], tok.to(DEV),
                         sd.lib.SD_RULE_SPEC, spec, spec, sd.PhiloxNoise(seed=bc.SEED, offset=bc.OFFSET),
                         torch.tensor(list(stops), dtype=torch.long, device=DEV), row_base=bc.ROW_BASE)


@pytest.mark.parametrize("name,V,dtype", [("multinomial", 4100, torch.bfloat16), ("topk50", 2049, torch.float32),
                                          ("greedy", 2047, torch.float16)])
def test_one_draft_equals_sd_verify(sd, name, V, dtype):
    """γ' = 1: h_1 = min(1, p/q), so n, the prune lengths, stop_index and the status are sd_verify's on
    the same inputs, seed and offset — and under greedy the token too.  (A stochastic token is drawn by
    inverse CDF on one uniform here and by sd_verify's own two-uniform draw there, as sd_verify_multi's
    at K = 1; resample_mass is the fp64 chunk-order sum here and an fp32 wave sum there: held to 1e-5.)"""
    c = bc.case(16, 1, V, dtype, name)
    stops = [int(c.tok[3, 0])]
    got = run_block(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, stops)
    one = _spec_verify(sd, c, c.tok, stops)
    for f in INT_FIELDS:
        assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f
    rej = (got.n_accepted == 0) & (got.stop_index < 0)
    assert int(rej.sum()) >= 2 and int((got.stop_index >= 0).sum()) >= 1
    assert torch.allclose(got.resample_mass[rej], one.resample_mass.cpu()[rej], rtol=0, atol=1e-5)
    if not c.proc.stochastic:
        assert torch.equal(got.next_token, one.next_token.cpu())


@pytest.mark.parametrize("g,V,dtype", [(4, 2049, torch.bfloat16), (32, 37, torch.float32)])
def test_ratios_of_at_least_one_equal_sd_verify(sd, g, V, dtype):
    """Every drafted token the one with the largest p/q of its row pair (>= 1): every w_t = 1, every
    h_t = 1, and both rules accept the whole block."""
    c = bc.case(16, g, V, dtype, "multinomial")
    P, Q = c.P.double().numpy(), c.Q.double().numpy()
    tok = torch.tensor([[int(np.nanargmax(bc._ratios(P[b], Q[b], t))) for t in range(g)] for b in range(c.B)])
    got = run_block(sd, c.tl.to(DEV), c.dl.to(DEV), tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE)
    one = _spec_verify(sd, c, tok, ())
    for f in INT_FIELDS:
        assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f
    assert torch.equal(got.n_accepted, torch.full((c.B,), g, dtype=torch.int32))
    assert torch.equal(got.weights, torch.ones(c.B, g + 1)) and torch.equal(got.accept_prob, torch.ones(c.B, g))


# ---------------------------------------------------------------- flagged rows
def test_out_of_range_ids_and_unusable_rows_are_flagged_never_sampled(sd):
    L = sd.lib
    c = bc.case(16, 4, 2049, torch.bfloat16, "multinomial")
    g, V = c.gamma, c.V
    # ids outside the vocabulary: p = q = 0, the ratio counts as +inf, the id stays in tokens_out
    tok = c.tok.clone()
    tok[0, 0], tok[1, 1] = -1, V
    c2 = SimpleNamespace(**{**vars(c), "tok": tok})
    rows = bc.host_results(c2, stops=())
    got = run_block(sd, c.tl.to(DEV), c.dl.to(DEV), tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE)
    check_case(sd, c2, got, rows)
    assert all(0 <= int(x) < V for x in got.next_token)
    # a NaN in the bonus row, and a bonus row that is `-inf` throughout, under sequences that accept the whole
    # block: torch.multinomial raises on such a row.  (A residual exit cannot meet an empty residual: the exit
    # at n is reached through an accepted test at n, h_n > 0, or at n = 0, where S_0 = 0 makes every later
    # weight 1 — the rule accepts deeper.)  The rows are flagged, emit their accepted drafts and no token;
    # every other sequence is bit-equal to the healthy call.
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    want = run_block(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, status_or=err)
    assert int(err.item()) == 0
    full = [b for b, r in enumerate(bc.host_results(c, stops=())) if r.status == br.BONUS and not r.close][:2]
    assert len(full) == 2
    tl = c.tl.clone()
    tl[full[0], g, V - 1] = float("nan")            # in the one-element last chunk
    tl[full[1], g, :] = -float("inf")
    got = run_block(sd, tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, status_or=err)
    for b in full:
        st = int(got.row_status[b])
        print(f"[block-flag] b={b} n={int(got.n_accepted[b])} status=0x{st:x} x={int(got.next_token[b])}")
        assert st & (L.SD_ROW_DONE | L.SD_ROW_ERROR_MASK) == L.SD_ROW_DONE | L.SD_ROW_INVALID_DIST, hex(st)
        assert int(got.next_token[b]) == -1 and int(got.n_accepted[b]) == g
        assert got.tokens_out[b].tolist() == c.tok[b].tolist() + [PAD]
    assert int(err.item()) == L.SD_ROW_INVALID_DIST
    rest = [b for b in range(c.B) if b not in full]
    for f in vars(want):
        assert torch.equal(getattr(got, f)[rest].nan_to_num(-1), getattr(want, f)[rest].nan_to_num(-1)), f


# ---------------------------------------------------------------- one workspace, many entry points
def test_one_workspace_serves_the_entry_points_in_turn(sd):
    """sd_verify_block, sd_verify, sd_sample and sd_verify_multi share the library's cached workspace
    at changing shapes; every block result equals the one computed first."""
    cases = [bc.case(16, 4, 2048, torch.float16, "multinomial"), bc.case(5, 2, 2049, torch.float16, "multinomial_T0.7", "none", "shifted")]
    first = [run_block(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, c.stops)
             for c in cases]
    m = mw.case(3, 4, 4, 4096, torch.bfloat16, "multinomial")
    for _ in range(2):
        for c, want in zip(cases, first):
            _spec_verify(sd, c, c.tok, c.stops)
            sd.ops.sample_rows(c.tl[:, 0].to(DEV).contiguous(), spec_of(sd, c.proc), sd.PhiloxNoise(seed=1))
            sd.ops.verify_multi(m.tl.to(DEV), m.dl.to(DEV), m.tok.to(DEV), spec_of(sd, m.proc), sd.PhiloxNoise(seed=2))
            got = run_block(sd, c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV), c.proc, bc.SEED, bc.OFFSET, bc.ROW_BASE, c.stops)
            for f in vars(want):
                assert torch.equal(getattr(got, f), getattr(want, f), ) or f == "resample_mass", f
            assert torch.equal(got.resample_mass.nan_to_num(-1), want.resample_mass.nan_to_num(-1))


# ---------------------------------------------------------------- graph capture
def test_graph_capture_replays_with_fresh_noise(sd):
    """Captured once with the Philox offset in device memory; each replay after offset_dev is bumped
    equals the eager call at that offset."""
    c = bc.case(16, 4, 2048, torch.float16, "multinomial")
    tl, dl, tok = c.tl.to(DEV), c.dl.to(DEV), c.tok.to(DEV)
    spec = spec_of(sd, c.proc)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    noise = sd.PhiloxNoise(seed=bc.SEED, offset=bc.OFFSET, offset_dev=off)
    stops = torch.empty(0, dtype=torch.long, device=DEV)
    sd.ops.verify_block(tl, dl, tok, spec, noise, stop_tokens=stops)          # warm: workspace allocated
    torch.cuda.synchronize()
    base = noise.offset                                                       # the host offset the capture takes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sd.ops.verify_block(tl, dl, tok, spec, noise, stop_tokens=stops)
    seen = set()
    for k in (0, 1, 5):
        off.fill_(k)
        graph.replay()
        torch.cuda.synchronize()
        want = sd.ops.verify_block(tl, dl, tok, spec, sd.PhiloxNoise(seed=bc.SEED, offset=base + k), stop_tokens=stops)
        for f in sd.ops.BLOCK_FIELDS:
            assert torch.equal(getattr(out, f).nan_to_num(-1), getattr(want, f).nan_to_num(-1)), (k, f)
        seen.add(tuple(out.n_accepted.tolist()))
    assert len(seen) >= 2                                                     # the noise did change


# ---------------------------------------------------------------- losslessness on the device
def _depth_rows(V, g, seed):
    """Depth-context rows: depth t has its own target and drafter row, shared by every sequence."""
    from oracle import specdec_ref as ref
    gen = torch.Generator().manual_seed(seed)
    tl = (torch.randn(g + 1, V, generator=gen) * 2).to(torch.bfloat16)
    dl = (tl[:g].float() + 0.8 * torch.randn(g, V, generator=gen)).to(torch.bfloat16)
    proc = mw.PROCS["multinomial"]
    return tl, dl, ref.process(tl, proc, exact=True).double().numpy(), ref.process(dl, proc, exact=True).double().numpy()


def _iid_batch(sd, tl, dl, q, B, seed):
    """One call on B sequences that share the rows tl [γ+1, V], dl [γ, V], drafts iid from the exact q."""
    g, V = dl.shape
    rng = np.random.default_rng(seed)
    tok = torch.from_numpy(np.stack([rng.choice(V, size=B, p=q[t] / q[t].sum()) for t in range(g)], axis=-1))
    T, D = tl.to(DEV), dl.to(DEV)
    out = sd.ops.verify_block([T[t].expand(B, V) for t in range(g + 1)], [D[t].expand(B, V) for t in range(g)],
                              tok.to(DEV), spec_of(sd, mw.PROCS["multinomial"]),
                              sd.PhiloxNoise(seed=seed * 7 + 1, offset=3), pad_token_id=PAD)
    assert not (out.row_status.cpu() & sd.lib.SD_ROW_ERROR_MASK).any()
    return out.tokens_out.cpu().numpy(), out.n_accepted.cpu().numpy(), rng


@pytest.mark.parametrize("g", [2, 4])
@pytest.mark.parametrize("V", [64, 1000])
def test_emitted_tokens_keep_the_target_distribution(sd, V, g):
    """4096 sequences on depth-context rows, drafts iid from the exact q on the host.  The first emitted
    token against the exact p_0; and the pair (t0, t1) against the exact pair distribution p_0 ⊗ p_1,
    where a sequence that emitted one token (n = 0) takes its second from the exact p_1 on the host, as
    the next step would: losslessness says the pair is the target's whatever the step accepted."""
    B = 4096
    tl, dl, p, q = _depth_rows(V, g, 17)
    emitted, n, rng = _iid_batch(sd, tl, dl, q, B, 100 + g)
    t0 = emitted[:, 0]
    assert t0.min() >= 0
    chi2_check(t0, p[0], f"block first token V={V} g={g}")
    one = n == 0
    assert one.sum() > B // 32 and (~one).sum() > B // 8
    t1 = emitted[:, 1].copy()
    t1[one] = rng.choice(V, size=int(one.sum()), p=p[1] / p[1].sum())
    chi2_check(t0 * V + t1, np.outer(p[0], p[1]).reshape(-1), f"block pairs V={V} g={g}")
    chi2_check(t1, p[1], f"block pairs' second token V={V} g={g}")
    assert (emitted[~one, 1] >= 0).all()


def test_mean_accepted_count_is_the_block_rules(sd):
    """One call at B = 16384 on the context-free pair of block_cases.stat_pair (V = 8, γ' = 4): the mean
    accepted count lies within 4 standard errors of the block rule's exact expectation; the CPU test
    asserts that this exceeds the token-wise expectation by more than 8 standard errors."""
    tl, dl, p, q = bc.stat_pair()
    eb, et, se = bc.stat_expectations()
    g = bc.STAT_GAMMA
    emitted, n, _ = _iid_batch(sd, tl[None].expand(g + 1, -1), dl[None].expand(g, -1), np.stack([q] * g), bc.STAT_B, 31)
    mean = float(n.mean())
    print(f"[block-stat] mean accepted {mean:.4f}, block expectation {eb:.4f}, token-wise {et:.4f}, se {se:.5f}")
    assert abs(mean - eb) <= 4 * se
