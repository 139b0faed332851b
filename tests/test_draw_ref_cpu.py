"""The host model of the PHILOX draw kernels (tests/draw_ref.py) on its own, without a GPU:

* the element order is chunk_elem's, a bijection, and what the kernels' loads imply;
* the models draw from the right distributions (chi-square over >= 50 000 (seed, row) pairs of one row);
* the checker has teeth: tokens of deliberately wrong models are rejected — the share per mutant is printed
  and must be at least half the rows on the near-flat input;
* the derived slacks stay under draw_ref.SLACK_CAP for every case of tests/test_gpu_draw_exact.py, and the
  conditions those cases put on their seeds hold (a second nucleus round, few close calls in the model).
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_ref as dr
import philox_ref as ph
from oracle import specdec_ref as ref
from test_gpu_draw import chi2_check

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# ---------------------------------------------------------------- Philox uniforms
def test_uniforms_match_their_definitions():
    seed, off, row = 0x1234_5678_9ABC_DEF0, (1 << 33) + 7, 70003
    for idx in (0, 1, 5, 129):
        x, y, z, _ = (int(w) for w in ph.block(seed, off, row, ph.SITE_CDF, idx))
        assert ph.cdf_uniform(seed, off, row, idx) == float(((x << 32) | y) >> 11) * 2.0 ** -53
        xn, yn, _, _ = (int(w) for w in ph.block(seed, off, row, 4, idx))
        assert ph.nuc_uniform(seed, off, row, idx) == float(((xn << 32) | yn) >> 11) * 2.0 ** -53
        if idx:
            u = np.float32(z >> 8) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
            g, E = ph.span_gumbel(seed, off, row, idx - 1)
            assert E == -math.log(float(u)) and g == -math.log(E)
    assert ph.cdf_uniform(seed, off, row) == ph.cdf_uniform(seed, off, row, 0)
    both = ph.cdf_uniform(seed, off, np.array([row, row + 1])[:, None], np.arange(3)[None, :])
    assert both.shape == (2, 3) and both[1, 2] == ph.cdf_uniform(seed, off, row + 1, 2)
    import vocab_parallel_ref as vp
    assert vp.cdf_uniform is ph.cdf_uniform


# ---------------------------------------------------------------- element order
@pytest.mark.parametrize("nst,vec", [(1, 8), (2, 8), (4, 8), (2, 4)])
def test_span_order_is_chunk_elems_bijection(nst, vec):
    ept, step = nst * vec, dr.THREADS * vec
    offs = dr.span_order(nst, vec)
    assert sorted(offs.tolist()) == list(range(dr.THREADS * ept))
    # chunk_elem, as the kernel writes it
    for pos in range(0, dr.THREADS * ept, 37):
        tid = pos // ept
        k = pos - tid * ept
        v = k // vec
        assert offs[pos] == (v * dr.THREADS + tid) * vec + (k - v * vec)
    # and from the loads: thread tid keeps the vector of stage v at v·STEP + tid·VEC in registers [v·VEC, (v + 1)·VEC)
    want = np.empty(dr.THREADS * ept, dtype=np.int64)
    for tid in range(dr.THREADS):
        for v in range(nst):
            for i in range(vec):
                want[tid * ept + v * vec + i] = v * step + tid * vec + i
    assert np.array_equal(offs, want)
    if nst == 1:
        assert np.array_equal(offs, dr.linear_order(nst, vec))


def test_spans_drop_elements_past_the_row_end():
    y = np.zeros(2056)
    for nst in (1, 2, 4):
        spans = dr.span_tables(y, nst, 8)
        assert sorted(np.concatenate([s.idx for s in spans]).tolist()) == list(range(2056))
        assert abs(sum(s.T for s in spans) - 2056) < 1e-9


# ---------------------------------------------------------------- distributions
N_DRAWS = 50_000


def one_row(V, dtype, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * scale).to(dtype)


def host_keep(x, proc):
    """(tau, tie_idx) of the exact oracle's keep set: the lowest kept value and the highest kept index
    that holds it (equal values are kept lowest index first)."""
    xf = x.float()
    exact = ref.processed_logits(xf.view(1, -1), dataclasses.replace(proc, stable_ties=True), exact=True)[0]
    kept = (exact > -1e19).numpy()
    v = dr.values32(x)
    tau = v[kept].min()
    return float(tau), int(np.nonzero(kept & (v == tau))[0].max())


def test_lean_model_draws_the_softmax():
    V, seeds = 4104, (11, 12)
    x = one_row(V, BF16, 5)
    tb = dr.lean_tables(x, BF16, 1)
    rows = np.arange(N_DRAWS // len(seeds), dtype=np.uint64)
    c = np.arange(len(tb.spans), dtype=np.uint64)
    toks = []
    for seed in seeds:
        U = ph.cdf_uniform(seed, 9, rows[:, None], c[None, :] + np.uint64(1))
        G, E = ph.span_gumbel(seed, 9, rows[:, None], c[None, :])
        toks += [dr.lean_decide(tb, U[i], G[i], E[i]).token for i in range(len(rows))]
        one = dr.lean_row(tb, seed, 9, 77)           # the per-row entry point reads the same words
        assert one.token == toks[-len(rows) + 77]
    chi2_check(toks, torch.softmax(x.double(), -1).numpy(), "lean model V=4104")


def test_draw_model_draws_the_processed_softmax():
    V, seeds = 4104, (21, 22)
    x = one_row(V, BF16, 6)
    proc = ref.Processor("topk", 0.8, 50)
    tb = dr.draw_tables(x, BF16, 0.8, host_keep(x, proc), 1)
    rows = np.arange(N_DRAWS // len(seeds), dtype=np.uint64)
    idx = np.arange(len(tb.spans) + 1, dtype=np.uint64)
    toks = []
    for seed in seeds:
        U = ph.cdf_uniform(seed, 2, rows[:, None], idx[None, :])
        toks += [dr.draw_decide(tb, U[i]).token for i in range(len(rows))]
        assert dr.draw_row(tb, seed, 2, 5).token == toks[-len(rows) + 5]
    probs = torch.softmax(torch.from_numpy(tb.y), -1).numpy()
    assert int((probs > 0).sum()) == 50
    chi2_check(toks, probs, "k_draw model topk50 T=0.8 V=4104")


def test_nuc_model_draws_the_nucleus_distribution():
    from test_gpu_draw import nucleus_case
    V, seed, T = 4104, 31, 0.7
    x = nucleus_case("peaked", V, BF16, 8)
    tb = dr.nuc_tables(x, BF16, T, 0.9)
    n = len(tb.slices)
    rows = np.arange(N_DRAWS, dtype=np.uint64)
    # round 0's uniforms in one Philox call; the rare later rounds by the model's own calls
    idx = (np.uint64(128) * np.arange(dr.NUC_K, dtype=np.uint64))[:, None] + np.arange(n + 1, dtype=np.uint64)[None, :]
    U0 = ph.nuc_uniform(seed, 4, rows[:, None, None], idx[None])

    def uniform(s, o, r, i):
        k = int(i[0]) // 128
        return U0[int(r), k] if k < dr.NUC_K else ph.nuc_uniform(s, o, r, i)

    toks, later = [], 0
    for r in range(N_DRAWS):
        m = dr.nuc_row(tb, seed, 4, r, uniform)
        assert m.token is not None
        toks.append(m.token)
        later += m.rounds > 1
    assert dr.nuc_row(tb, seed, 4, 123).token == toks[123]
    want = np.where(tb.kept, np.exp(tb.y - tb.y.max()), 0.0)
    print(f"[draw-ref] nucleus model: {int(tb.kept.sum())} kept, {later} of {N_DRAWS} draws needed a later round")
    chi2_check(toks, want / want.sum(), "k_draw_nuc model peaked V=4104 top_p=0.9 T=0.7")


# ---------------------------------------------------------------- the checker has teeth
TEETH_V, TEETH_ROWS, TEETH_OFFS = 12296, 24, (3, 4)


def shifted_uniform(seed, off, row, idx):
    """span c drawn with span c + 1's uniform (idx 0, the row's own, stays)."""
    idx = np.asarray(idx, dtype=np.uint64)
    return ph.cdf_uniform(seed, off, row, np.where(idx > 0, idx + np.uint64(1), idx))


def no_gumbel(seed, off, row, c):
    return np.zeros(len(c)), np.ones(len(c))


def neighbour(tok, V):
    return tok + 1 if tok + 1 < V else tok - 1


def rejected_share(kind, tables, model, check, mutant):
    """The share of (row, offset) pairs whose mutant token the checker turns down."""
    x, _ = dc.make_rows(TEETH_ROWS, TEETH_V, BF16, 99, 2048, (kind,))
    bad = n = 0
    for r in range(TEETH_ROWS):
        tb = tables(x[r])
        for off in TEETH_OFFS:
            tok = mutant(x[r], tb, off, r)
            ok, _, _, _ = check(tb, model(tb, 1717, off, r), tok)
            bad += not ok
            n += 1
    return bad / n


LEAN_MUTANTS = {
    "linear order, NST 2": (2, lambda x, tb, off, r: dr.lean_row(dr.lean_tables(x, BF16, 2, dr.linear_order), 1717, off, r).token),
    "linear order, NST 4": (4, lambda x, tb, off, r: dr.lean_row(dr.lean_tables(x, BF16, 4, dr.linear_order), 1717, off, r).token),
    "neighbouring element": (1, lambda x, tb, off, r: neighbour(dr.lean_row(tb, 1717, off, r).token, TEETH_V)),
    "span c on span c+1's uniform": (1, lambda x, tb, off, r: dr.lean_row(tb, 1717, off, r, uniform=shifted_uniform).token),
    "row r on row r+1's blocks": (1, lambda x, tb, off, r: dr.lean_row(tb, 1717, off, r + 1).token),
    "offset + 1": (1, lambda x, tb, off, r: dr.lean_row(tb, 1717, off + 1, r).token),
    "race without the Gumbel term": (1, lambda x, tb, off, r: dr.lean_row(tb, 1717, off, r, gumbel=no_gumbel).token),
}

DRAW_MUTANTS = {
    "linear order, nst 2": (2, lambda x, tb, off, r: dr.draw_row(dr.draw_tables(x, BF16, 0.7, None, 2, dr.linear_order), 1717, off, r).token),
    "neighbouring element": (1, lambda x, tb, off, r: neighbour(dr.draw_row(tb, 1717, off, r).token, TEETH_V)),
    "span c on span c+1's uniform": (1, lambda x, tb, off, r: dr.draw_row(tb, 1717, off, r, uniform=shifted_uniform).token),
    "row r on row r+1's blocks": (1, lambda x, tb, off, r: dr.draw_row(tb, 1717, off, r + 1).token),
    "offset + 1": (1, lambda x, tb, off, r: dr.draw_row(tb, 1717, off + 1, r).token),
}


def second_kept(tb, off, r):
    kept = [q.token for q in dr.nuc_proposals(tb, 1717, off, r) if q.kept]
    return kept[1] if len(kept) > 1 else -1


@pytest.mark.parametrize("name", list(LEAN_MUTANTS))
def test_checker_rejects_wrong_lean_models(name):
    nst, mutant = LEAN_MUTANTS[name]
    shares = {kind: rejected_share(kind, lambda x: dr.lean_tables(x, BF16, nst), dr.lean_row, dr.check_lean, mutant)
              for kind in ("flat", "normal")}
    print(f"[draw-ref] mutant k_draw_lean / {name}: rejected {shares['flat']:.0%} of near-flat rows, "
          f"{shares['normal']:.0%} of N(0, 3^2) rows")
    assert shares["flat"] >= 0.5


@pytest.mark.parametrize("name", list(DRAW_MUTANTS))
def test_checker_rejects_wrong_draw_models(name):
    nst, mutant = DRAW_MUTANTS[name]
    shares = {kind: rejected_share(kind, lambda x: dr.draw_tables(x, BF16, 0.7, None, nst), dr.draw_row, dr.check_draw,
                                   mutant) for kind in ("flat", "normal")}
    print(f"[draw-ref] mutant k_draw / {name}: rejected {shares['flat']:.0%} of near-flat rows, "
          f"{shares['normal']:.0%} of N(0, 3^2) rows")
    assert shares["flat"] >= 0.5


def test_checker_rejects_the_second_kept_proposal():
    shares = {kind: rejected_share(kind, lambda x: dr.nuc_tables(x, BF16, 1.0, 0.5), dr.nuc_row, dr.check_nuc,
                                   lambda x, tb, off, r: second_kept(tb, off, r)) for kind in ("flat", "normal")}
    print(f"[draw-ref] mutant k_draw_nuc / second kept proposal: rejected {shares['flat']:.0%} of near-flat rows, "
          f"{shares['normal']:.0%} of N(0, 3^2) rows")
    assert shares["flat"] >= 0.5


def test_checker_accepts_the_model_itself():
    x, _ = dc.make_rows(8, TEETH_V, BF16, 99, 2048)
    for r in range(8):
        for tables, model, check in ((lambda v: dr.lean_tables(v, BF16, 2), dr.lean_row, dr.check_lean),
                                     (lambda v: dr.draw_tables(v, BF16, 0.7, None, 1), dr.draw_row, dr.check_draw),
                                     (lambda v: dr.nuc_tables(v, BF16, 0.7, 0.9), dr.nuc_row, dr.check_nuc)):
            tb = tables(x[r])
            m = model(tb, 5, 6, r)
            ok, _, used, _ = check(tb, m, m.token)
            assert ok and used == 0.0


# ---------------------------------------------------------------- the GPU cases' conditions
CPU_ROWS = 16      # rows per case modelled here (the GPU test models every row)


def case_keep(c, x):
    if c.proc == "multinomial":
        return None
    return host_keep(x, ref.Processor(c.proc, c.T, c.top_k, c.top_p))


def test_slack_cap_holds_for_every_gpu_case():
    worst = {}
    for c in dc.lean_cases() + dc.draw_cases() + dc.nuc_cases():
        x, _ = dc.case_rows(c)
        for r in range(c.B):
            if c.kernel == "lean":
                tb = dr.lean_tables(x[r], c.dtype, dr.lean_nst(c.B, c.pin))
            elif c.kernel == "draw":
                tb = dr.draw_tables(x[r], c.dtype, c.T, case_keep(c, x[r]), dr.draw_nst(c.B, c.V, c.dtype))
            else:
                tb = dr.nuc_tables(x[r], c.dtype, c.T, c.top_p)
            inner, outer = dr.slack_shares(tb)
            assert inner <= dr.SLACK_CAP and outer <= dr.SLACK_CAP, (c.id, r, inner, outer)
            key = (c.kernel, dc.dt_name(c.dtype))
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], inner), max(w[1], outer))
    print("[draw-ref] slack cap 1e-5: largest slack / total per kernel and dtype (in-span, span pick)")
    for (kernel, dt), (inner, outer) in sorted(worst.items()):
        print(f"[draw-ref]   {kernel:5s} {dt}: {inner:.3g}  {outer:.3g}")


def test_lean_model_flags_few_races():
    """The model alone: race close calls (two keys within tol) stay far under the cap on the cases' seeds."""
    rows = close = 0
    least = math.inf
    for c in dc.lean_cases():
        x, _ = dc.case_rows(c)
        for r in range(min(c.B, CPU_ROWS)):
            tb = dr.lean_tables(x[r], c.dtype, dr.lean_nst(c.B, c.pin))
            for off, rb in zip(c.offsets, c.row_bases):
                m = dr.lean_row(tb, c.noise_seed, off, rb + r)
                assert m.token >= 0
                rows += 1
                close += m.close
                least = min(least, m.gap)
    print(f"[draw-ref] k_draw_lean model: {close} race close calls in {rows} rows, smallest key gap {least:.3g}")
    assert close <= dr.CLOSE_CAP * rows


@pytest.mark.parametrize("c", dc.nuc_cases(), ids=lambda c: c.id)
def test_nucleus_case_seeds(c):
    """Every row's model keeps a proposal; at top_p = 0.5 some row needs a second round, at 0.9 some row
    a proposal after its first; close keep decisions stay under the cap."""
    x, _ = dc.case_rows(c)
    tabs = [dr.nuc_tables(x[r], c.dtype, c.T, c.top_p) for r in range(c.B)]
    rounds = later_k = close = n = 0
    for off, rb in zip(c.offsets, c.row_bases):
        for r in range(c.B):
            m = dr.nuc_row(tabs[r], c.noise_seed, off, rb + r)
            assert m.token is not None, (off, r)
            rounds = max(rounds, m.rounds)
            later_k += m.first_k > 0 or m.rounds > 1
            close += m.close
            n += 1
    print(f"[draw-ref] {c.id}: rounds needed {rounds}, {later_k} of {n} rows past their first proposal, {close} close")
    assert rounds >= 2 if c.top_p == 0.5 else later_k > 0
    assert close <= dr.CLOSE_CAP * n
