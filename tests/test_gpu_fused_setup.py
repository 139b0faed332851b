"""The block-id fused verify, whose workgroups now split their block id into (sequence, slot, span), decider
or sampler by multiplying with host-computed reciprocals (csrc/sd_index.h, stats_body), at every decided
slot, row layout, dtype and rule.

Two more changes to its set-up were measured and parked as patches (DESIGN.md section 6,
scripts/experiments/): the samplers looking every slot's rows and their alignment up while they wait for
the decision (fused_sampler_early_rows.patch) and the decider forming the drafter side of every draft's
ratio before the span records (decider_early_drafter_side.patch).  The per-slot alignment, layout and
decider cases below hold pair_rows and decide_seq as they stand and are the guard for either patch.

None of this may change a bit.  Every fused call here is compared with the two-launch verify (k_stats +
k_sample, SD_OPT_FUSED_VERIFY = 0) on the same inputs, Philox seed and offsets: exact equality of every
output field, of row_counts and of the engine state, and every call asserts the path it took.  The helpers
are tests/test_gpu_fused_tail.py's.  Shapes: B = 8 and 16, 2048-element chunks, two per sampler, so V in
{2048, 2056, 6152, 10248} gives one chunk, a second chunk of 8 elements, four chunks with a ragged last one
and six; with gamma = 4 row b is driven to decide at slot b % 5 (4: every draft accepted), so every call
has every decided slot, which the test asserts from n_accepted."""
import pytest
import torch

from test_gpu_fused_tail import (DEV, Step, assert_same, check_decided, laid_out, logits, once, rows_of, three_eager,
                                 three_replays, emitted)

pytestmark = pytest.mark.gpu
G = 4
VOCABS = [2048, 2056, 6152, 10248]


def drive(tl, dl, want):
    """Edits tl / dl so that row b decides at slot want[b] (>= the draft count: every draft accepted): the
    drafter rows before it equal the target rows (p / q = 1 > u), and the draft there is the drafter's
    likeliest token, raised to q ~ 1, with no mass under the target.  Returns the draft override."""
    B, g = dl.shape[0], dl.shape[1]
    mask = torch.zeros(B, g, dtype=torch.bool, device=DEV)
    tok = torch.zeros(B, g, dtype=torch.long, device=DEV)
    for b in range(B):
        i = min(int(want[b]), g)
        dl[b, :i] = tl[b, :i]
        if i < g:
            k = int(dl[b, i].float().argmax())
            dl[b, i, k] += 12.0
            tl[b, i, k] = -100.0
            mask[b, i], tok[b, i] = True, k
    return mask, tok


def n_accepted_is(res, want, g):
    assert res["n_accepted"].tolist() == [min(int(w), g) for w in want], (res["n_accepted"].tolist(), list(want))


# ---------------------------------------------------------------- shapes, dtypes, rules: every decided slot
@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B", [8, 16])
def test_every_decided_slot(B, dt, rule):
    from specdec_amd import _lib
    for V in VOCABS:
        seed = 5 * B + V % 89 + {"bf16": 0, "fp16": 1, "fp32": 2}[dt] + (40 if rule == "spec" else 0)
        tl, dl = logits(B, G, V, dt, seed)
        want = [b % 5 for b in range(B)]
        override = drive(tl, dl, want)
        step = Step(*rows_of(tl, dl, rule), rule, engine=rule == "engine", draft_override=override)
        two = once(step, "two", seed)
        n_accepted_is(two, want, G)
        check_decided(two, rule, B)
        rej = [b for b in range(B) if want[b] < G]
        assert (two["row_status"][rej] & _lib.SD_ROW_RESIDUAL).all()
        assert ((two["next_token"][rej] >= 0) & (two["next_token"][rej] < V)).all()
        if rule == "spec":   # every draft accepted: the bonus row, slot gamma
            assert (two["row_status"][[b for b in range(B) if want[b] == G]] & _lib.SD_ROW_BONUS).all()
        assert_same(once(step, "fused", seed), two, (V,))


# ---------------------------------------------------------------- row layouts
def spaced(x, way):
    """The rows [B, V] of x [B, T, V]: 'views' (equally spaced), or 'separate' (tests/test_gpu_fused_tail.py)."""
    return laid_out(x, way)


LAYOUTS = {"views": ("views", "views", 1), "separate": ("separate", "separate", 1), "target-even": ("views", "separate", 1),
           "drafter-even": ("separate", "views", 1), "alias": ("alias", "alias", 1), "arg-fast-0": ("views", "views", 0)}


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_row_layouts(name, rule):
    B, V = 8, 6152
    t_way, d_way, fast = LAYOUTS[name]
    tl, dl = logits(B, G, V, "bf16", 301)
    n_t = G + (1 if rule == "spec" else 0)
    want = [b % 5 for b in range(B)]
    override = None if name == "alias" else drive(tl, dl, want)   # one tensor for every slot: whatever it decides
    step = Step(laid_out(tl[:, :n_t], t_way), laid_out(dl, d_way), rule, engine=rule == "engine", draft_override=override)
    if name in ("target-even", "drafter-even"):
        gaps = lambda rows: {rows[t + 1].data_ptr() - rows[t].data_ptr() for t in range(len(rows) - 1)}
        even, uneven = (step.trows, step.drows) if name == "target-even" else (step.drows, step.trows)
        assert len(gaps(even)) == 1 and len(gaps(uneven)) > 1
    two = once(step, "two", 302)
    check_decided(two, rule, B)
    if override is not None:
        n_accepted_is(two, want, G)
    assert_same(once(step, "fused", 302, arg_fast=fast), two, name)


def shifted(x, shifts):
    """The rows [B, V] of x [B, T, V], every slot in a buffer of its own at a 16-byte row stride, slot t
    starting shifts[t] elements past a 16-byte boundary."""
    B, T, V = x.shape
    S = (V + 7) // 8 * 8
    rows = []
    for t in range(T):
        buf = torch.zeros(B * S + 8, dtype=x.dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[shifts[t]:shifts[t] + B * S].view(B, S)[:, :V]
        view.copy_(x[:, t])
        rows.append(view)
    return rows


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("side", ["target", "drafter"])
def test_slot_alignment_mask(side, rule):
    """Slot 0 starts on a 16-byte boundary and slot 1 one element later, on the target rows or on the
    drafter rows: a decision at slot 1 takes the samplers' one-chunk-at-a-time path, one at slot 0 the
    vector path, whichever came first."""
    B, V = 8, 6152
    n_t = G + (1 if rule == "spec" else 0)
    for slot in (1, 0):
        tl, dl = logits(B, G, V, "bf16", 311 + slot)
        want = [slot] * B
        override = drive(tl, dl, want)
        t_sh = [1 if t == 1 and side == "target" else 0 for t in range(n_t)]
        d_sh = [1 if t == 1 and side == "drafter" else 0 for t in range(G)]
        trows, drows = shifted(tl[:, :n_t], t_sh), shifted(dl, d_sh)
        odd = (trows if side == "target" else drows)
        assert odd[0].data_ptr() % 16 == 0 and odd[1].data_ptr() % 16 == 2
        step = Step(trows, drows, rule, engine=rule == "engine", draft_override=override)
        two = once(step, "two", 313)
        n_accepted_is(two, want, G)
        check_decided(two, rule, B)
        assert_same(once(step, "fused", 313), two, (side, slot))


# ---------------------------------------------------------------- the decider's early drafter side
@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_decider_cases(dt, rule):
    """row 0: draft 1's token has a drafter probability that rounds to 0 (logit -100; the target's too):
      q <= 0 accepts under the engine rule, and u > 0 / 0 is false under the reference's;
    row 1: draft 2's id lies past the vocabulary, row 2: it is negative (p = q = 0, the same tests);
    row 3: every draft accepted with the stop token at draft 1;
    rows 4, 5: inactive (engine rule);
    rows 6, 7: random rows."""
    from specdec_amd import _lib
    B, V = 8, 6152
    tl, dl = logits(B, G, V, dt, 321)
    dl[0:4] = tl[0:4, :G]
    mask = torch.zeros(B, G, dtype=torch.bool, device=DEV)
    tok = torch.zeros(B, G, dtype=torch.long, device=DEV)
    kz = 4100
    tl[0, 1, kz] = -100.0
    dl[0, 1, kz] = -100.0
    mask[0, 1], tok[0, 1] = True, kz
    mask[1, 2], tok[1, 2] = True, V + 5
    mask[2, 2], tok[2, 2] = True, -3
    stop_tok = 77
    mask[3, 1], tok[3, 1] = True, stop_tok
    tl[3, 1, stop_tok] = 30.0      # p = q ~ 1 at the stop token: accepted
    dl[3, 1, stop_tok] = 30.0
    active = torch.tensor([1, 1, 1, 1, 0, 0, 1, 1], dtype=torch.uint8, device=DEV) if rule == "engine" else None
    step = Step(*rows_of(tl, dl, rule), rule, engine=rule == "engine", active=active, draft_override=(mask, tok),
                stop=torch.tensor([stop_tok], device=DEV))
    two = once(step, "two", 322)
    n, st = two["n_accepted"], two["row_status"]
    assert n[0] == G and n[1] == G and n[2] == G, n.tolist()
    if rule == "engine":
        assert n[3] == 2 and (st[3] & _lib.SD_ROW_FINISHED)          # ends at its first accepted stop token
        assert not (st[4:6] & _lib.SD_ROW_DONE).any()
    else:
        assert (st[3] & _lib.SD_ROW_STOP_IN_DRAFTS) and two["stop_index"][3] == 1
    assert_same(once(step, "fused", 322), two)


# ---------------------------------------------------------------- row_counts over calls and replays
def test_three_eager_calls_and_three_replays():
    B, V = 8, 6152
    tl, dl = logits(B, G, V, "bf16", 331)
    override = drive(tl, dl, [b % 5 for b in range(B)])
    step = Step(*rows_of(tl, dl, "engine"), "engine", engine=True, draft_override=override)
    two = three_eager(step, "two", 332)
    for name, snaps in {"eager": three_eager(step, "fused", 332), "graph": three_replays(step, 332)}.items():
        total = torch.zeros(B, 2, dtype=torch.long)
        for i in range(3):
            assert_same(snaps[i], two[i], (name, i))
            total += emitted(snaps[i])
            assert torch.equal(snaps[i]["counts"], total), (name, i)
        assert total[:, 1].sum() > total[:, 0].sum() > 0
    assert not torch.equal(two[0]["next_token"], two[1]["next_token"])
