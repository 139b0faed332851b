"""sd_verify_multi at the edges of its inputs (its row loads, token loads and draw are code of this
path alone):

* vocabularies below, at and above one 16-byte vector and one wave, rows handed over as the list
  form (γ+1 tensors [B*K, V]) in the layouts of tests/row_edges.py — packed, padded, shifted —
  each depth in its own buffer with +inf or NaN around every row, `-inf` entries inside the rows,
  a draft_tokens row longer than γ, and the draws' statistics at a row stride above B·K;
* flagged rows: a bonus row without a distribution (NaN, or all `-inf`);
* drafted ids outside the vocabulary, and chains with identical drafts.

Every case is checked row by row against the host model as tests/test_gpu_multidraft.py's
(check_case, the draw's interval included); tests/test_multidraft_cpu.py proves what the cases reach.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import multi_walk as mw
import multidraft_ref as mref
import row_edges as rowe
from test_gpu_multidraft import PAD, check_case, spec_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPARE = 5               # rows of the hints beyond B·K


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise)


def fields(sd, out):
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in sd.ops.MULTI_FIELDS}, tokens_out=out.tokens_out.cpu())


def depth_rows(x, place):
    """The list form of x [B, K, n, V]: per depth a [B*K, V] tensor, each placed on its own."""
    B, K, n, V = x.shape
    return [place(x[:, :, t].reshape(B * K, V)) for t in range(n)]


def spare_hints(sd, drows, proc):
    """(stats [γ, R + SPARE, 2], keeps [γ, R + SPARE, 4] or None) of the placed drafter rows as
    sample_rows returns them with its draws; the spare rows hold NaN / -1."""
    g, R = len(drows), drows[0].shape[0]
    spec = spec_of(sd, proc)
    stats = torch.full((g, R + SPARE, 2), math.nan, device=DEV)
    keeps = torch.full((g, R + SPARE, 4), -1, dtype=torch.int32, device=DEV) if spec.keeps else None
    noise = sd.PhiloxNoise(seed=4242)
    for d in range(g):
        sd.ops.sample_rows(drows[d], spec, noise, row_stats_out=stats[d, :R],
                           row_keep_out=keeps[d, :R] if keeps is not None else None)
    assert bool(stats[:, R:].isnan().all()) and (keeps is None or bool((keeps[:, R:] == -1).all()))
    return stats, keeps


def run_list(sd, c, tok, place=None, hinted=False, stops=(), status_or=None, tl=None, dl=None):
    """verify_multi on the list form of case c's rows (tl / dl: replacements of c.tl / c.dl)."""
    place = place or (lambda t: t.contiguous().to(DEV))
    trows = depth_rows(c.tl if tl is None else tl, place)
    drows = depth_rows(c.dl if dl is None else dl, place)
    kw = {}
    if hinted:
        kw["draft_row_stats"], kw["draft_row_keep"] = spare_hints(sd, drows, c.proc)
    out = sd.ops.verify_multi(trows, drows, tok.to(DEV), spec_of(sd, c.proc), sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET),
                              num_drafts=c.K, stop_tokens=torch.tensor(list(stops), dtype=torch.long, device=DEV),
                              row_base=mw.ROW_BASE, pad_token_id=PAD, status_or=status_or, **kw)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_MULTI
    return fields(sd, out)


# ---------------------------------------------------------------- small vocabularies, row layouts
def _small_id(case):
    B, K, g, V, dtype, name, mask, layout, hinted = case
    return f"K{K}-g{g}-V{V}-{rowe.dt_name(dtype)}-{name}-{mask}-{layout}" + ("-hinted" if hinted else "")


@pytest.mark.parametrize("case", mw.small_grid(), ids=_small_id)
def test_small_vocabularies_and_row_layouts_equal_the_host_model(sd, case):
    B, K, g, V, dtype, name, mask, layout, hinted = case
    c = mw.small_case(*case[:7])
    rows = mw.host_results(c)
    poison = rowe.poison_of(layout, "multi", V, K, g, rowe.dt_name(dtype), name, mask)
    place = lambda t: rowe.place(t, layout, poison, DEV)      # noqa: E731
    # a draft_tokens row longer than γ: the columns past γ hold ids no row has
    tok = torch.full((B * K, g + 3), V + 7, dtype=torch.long)
    tok[:, :g] = c.tok.reshape(B * K, g)
    got = run_list(sd, c, tok[:, :], place, hinted)
    check_case(sd, c, got, rows)
    if V == 1:
        assert all(r.status == mref.BONUS for r in rows)
        assert torch.equal(got.tokens_out, torch.zeros(B, g + 1, dtype=torch.long))


# ---------------------------------------------------------------- flagged rows
FLAG_SHAPE = (4, 2, 2, 2049, torch.bfloat16, "multinomial")
BAD = 1


def _status_word():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _assert_rows_equal(sd, a, b, rows_):
    for f in sd.ops.MULTI_FIELDS + ("tokens_out",):
        x, y = getattr(a, f)[rows_], getattr(b, f)[rows_]
        if x.is_floating_point():
            x, y = torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)
        assert torch.equal(x, y), f


@pytest.mark.parametrize("bad", ["nan", "all-minus-inf"])
def test_bonus_row_without_a_distribution_is_flagged(sd, bad):
    """Sequence 1 accepts every draft (its drafter rows equal its target rows: every ratio is 1) and
    its winner's bonus row holds a NaN, or is `-inf` throughout: torch.multinomial raises on such a
    row.  The row is flagged, emits its accepted drafts and no token; the other sequences are
    bit-equal to the call in which sequence 1's bonus row is healthy."""
    L = sd.lib
    c = mw.case(*FLAG_SHAPE)
    B, K, g, V = c.B, c.K, c.gamma, c.V
    tl, dl = c.tl.clone(), c.dl.clone()
    dl[BAD] = tl[BAD, :, :g]
    healthy = SimpleNamespace(**{**vars(c), "tl": tl, "dl": dl, "P": c.P.clone(), "Q": c.Q.clone()})
    healthy.Q[BAD] = healthy.P[BAD, :, :g]
    rows = mw.host_results(healthy)
    assert rows[BAD].status == mref.BONUS and rows[BAD].n == g and rows[BAD].winner == 0
    err = _status_word()
    want = run_list(sd, healthy, c.tok.reshape(B * K, g), status_or=err)
    check_case(sd, healthy, want, rows)
    assert int(err.item()) == 0

    broken = tl.clone()
    if bad == "nan":
        broken[BAD, 0, g, V - 1] = math.nan          # in the one-element last chunk
    else:
        broken[BAD, 0, g, :] = -math.inf
    got = run_list(sd, healthy, c.tok.reshape(B * K, g), status_or=err, tl=broken)
    st = int(got.row_status[BAD])
    assert st & (L.SD_ROW_DONE | L.SD_ROW_ERROR_MASK) == L.SD_ROW_DONE | L.SD_ROW_INVALID_DIST, hex(st)
    assert int(got.next_token[BAD]) == -1
    assert int(got.n_accepted[BAD]) == g and int(got.winner[BAD]) == 0
    assert got.tokens_out[BAD].tolist() == c.tok[BAD, 0].tolist() + [PAD]
    assert int(err.item()) == L.SD_ROW_INVALID_DIST
    _assert_rows_equal(sd, got, want, [b for b in range(B) if b != BAD])

    # the same row under a chain that does not win is never drawn from: nothing is flagged
    other = tl.clone()
    other[BAD, 1, g, :] = broken[BAD, 0, g, :]
    err2 = _status_word()
    got2 = run_list(sd, healthy, c.tok.reshape(B * K, g), status_or=err2, tl=other)
    assert int(err2.item()) == 0
    _assert_rows_equal(sd, got2, want, list(range(B)))


def test_nan_target_row_accepts_like_the_host_model(sd):
    """A NaN in a target row under test makes every ratio of that row NaN, and `u > NaN` is false:
    the draft is accepted (as sd_verify's SPEC rule and the reference's `r > p / q`), the walk goes
    on at the next depth and nothing is flagged unless the draw itself meets such a row."""
    c = mw.case(*FLAG_SHAPE)
    B, K, g, V = c.B, c.K, c.gamma, c.V
    free = mw.host_results(c)
    assert free[BAD].n == 0 and free[BAD].status == mref.RESIDUAL      # scenario rej0
    tl = c.tl.clone()
    tl[BAD, 0, 0, 3] = math.nan
    sick = SimpleNamespace(**{**vars(c), "tl": tl, "P": c.P.clone()})
    sick.P[BAD, 0, 0] = math.nan
    rows = mw.host_results(sick)
    assert rows[BAD].n >= 1
    err = _status_word()
    got = run_list(sd, sick, c.tok.reshape(B * K, g), status_or=err)
    r = rows[BAD]
    ints = tuple(int(getattr(got, f)[BAD]) for f in ("n_accepted", "winner", "n_sibling_rejects", "prune_drafter",
                                                    "prune_target", "stop_index"))
    assert ints == (r.n, r.winner, r.rejects, r.prune_drafter, r.prune_target, r.stop_index) or r.close
    assert int(err.item()) == 0 and not int(got.row_status[BAD]) & sd.lib.SD_ROW_ERROR_MASK
    want = run_list(sd, c, c.tok.reshape(B * K, g))
    _assert_rows_equal(sd, got, want, [b for b in range(B) if b != BAD])


# ---------------------------------------------------------------- drafted ids outside the vocabulary
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("bad_id", ["minus-one", "V"])
@pytest.mark.parametrize("K", [1, 4])
def test_out_of_range_draft_id_is_accepted_like_the_host_model(sd, K, bad_id, depth):
    """A drafted id outside [0, V) has p = q = 0: its ratio is NaN and the test accepts, as the host
    model's (frac = NaN) and sd_verify's.  Sequence b's chain b % K holds the id; it reaches
    tokens_out unchanged where that chain wins; with one chain every integer output equals
    sd_verify(SD_RULE_SPEC)'s on the same inputs."""
    c0 = mw.case(16, K, 2, 1000, torch.bfloat16, "multinomial")
    B, g, V = c0.B, c0.gamma, c0.V
    bad = -1 if bad_id == "minus-one" else V
    tok = c0.tok.clone()
    for b in range(B):
        tok[b, b % K, depth] = bad
    c = SimpleNamespace(**{**vars(c0), "tok": tok})
    rows = mw.host_results(c)
    assert sum(r.close for r in rows) <= 1
    taken = [b for b, r in enumerate(rows) if bad in r.accepted]
    assert len(taken) >= 3
    got = run_list(sd, c, tok.reshape(B * K, g))
    # check_case's row[:n] == tok[winner, :n] holds the id to its place; the emitted x stays inside [0, V)
    check_case(sd, c, got, rows)
    same = [b for b in taken if int(got.n_accepted[b]) == rows[b].n and int(got.winner[b]) == rows[b].winner]
    assert len(same) >= len(taken) - 1
    assert all(bad in got.tokens_out[b, :rows[b].n].tolist() for b in same)
    if K == 1:
        spec = spec_of(sd, c.proc)
        tl, dl = c.tl[:, 0].to(DEV), c.dl[:, 0].to(DEV)
        one = sd.ops.verify([tl[:, t] for t in range(g + 1)], [dl[:, t] for t in range(g)], tok[:, 0].to(DEV),
                            sd.lib.SD_RULE_SPEC, spec, spec, sd.PhiloxNoise(seed=mw.SEED, offset=mw.OFFSET),
                            row_base=mw.ROW_BASE)
        for f in ("n_accepted", "prune_drafter", "prune_target", "stop_index", "row_status"):
            assert torch.equal(getattr(got, f), getattr(one, f).cpu()), f


# ---------------------------------------------------------------- identical chains
def test_chains_with_identical_drafts_stay_alive_together(sd):
    """Chains 0 and 1 (and 2 and 3) hold the same drafts: an accept keeps both in the alive set, a
    reject of the first leaves the second a zero residual at that token (it is rejected too), and the
    winner is the lower index."""
    c0 = mw.case(16, 4, 2, 1000, torch.bfloat16, "multinomial")
    tok = c0.tok.clone()
    tok[:, 1] = tok[:, 0]
    tok[:, 3] = tok[:, 2]
    c = SimpleNamespace(**{**vars(c0), "tok": tok})
    rows = mw.host_results(c)
    assert sum(r.close for r in rows) <= 1
    assert all(r.winner in (0, 2) for r in rows)
    assert sum(r.status == mref.BONUS for r in rows) >= 2 and sum(r.winner == 2 for r in rows) >= 1
    # a rejected token's twin is tested against a zero residual
    assert any(frac == 0.0 and not acc for r in rows for d, k, j, frac, acc in r.tests if k in (1, 3))
    got = run_list(sd, c, tok.reshape(c.B * c.K, c.gamma))
    check_case(sd, c, got, rows)
    assert all(int(w) in (0, 2) for w in got.winner)
