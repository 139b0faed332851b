"""The fused verify's tail after its reordering (csrc/specdec_kernels.hip): the finisher fetches the row
counters beside the engine state before the chunk pick (finalize_early), and the decider's lane sends the
samplers' decision records before its bookkeeping (walk_decision).  The same cases hold a build with
SD_SAMP_TOTALS_FIRST = 1 (a block-id sampler's two totals records before either in-chunk walk,
fused_pair_pick: parked) to the same outputs.

None of this may change a bit.  Every fused call here is compared with the two-launch verify
(k_stats + k_sample, SD_OPT_FUSED_VERIFY = 0) on the same inputs, Philox seed and offsets: exact
equality of every output field, of row_counts and of the engine state, and every call asserts the
path it took (sd_last_verify_path).  The shapes are the smallest that reach each branch: 2048-element
chunks, two per sampler, so V in {2048 .. 10248} gives a sampler without a second chunk, a second
chunk of 8 elements, even and odd chunk counts and a ragged last chunk."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OUT_FIELDS = ("n_accepted", "next_token", "row_status", "resample_mass", "stop_index", "prune_drafter", "prune_target")


def opt(name, value):
    from specdec_amd import _lib
    return _lib.option(getattr(_lib, name), value)


@contextlib.contextmanager
def path(kind, arg_fast=1, ticket=-1, samp_chunks=0):
    """kind: 'fused' or 'two' (the lean one-workgroup verify of small batches off in both)."""
    with opt("SD_OPT_LEAN_VERIFY", 0), opt("SD_OPT_FUSED_VERIFY", 1 if kind == "fused" else 0), \
            opt("SD_OPT_ARG_FAST", arg_fast), opt("SD_OPT_FUSED_TICKET", ticket), opt("SD_OPT_SAMP_CHUNKS", samp_chunks):
        yield


def logits(B, g, V, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    tl = (torch.randn(B, g + 1, V, generator=gen) * 3).to(DTYPES[dt])
    dl = (tl[:, :g].float() + torch.randn(B, g, V, generator=gen)).to(DTYPES[dt])
    return tl.to(DEV), dl.to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k, a[k], b[k])


class Step:
    """One verify step's tensors: the draws of the drafter rows (tokens, row stats), then the verify."""

    def __init__(self, trows, drows, rule, engine=False, active=None, counts=True, draft_override=None, stop=None):
        from specdec_amd import _lib, ops
        self.trows, self.drows = list(trows), list(drows)
        self.g, self.B = len(self.drows), self.drows[0].shape[0]
        self.rule = _lib.SD_RULE_SPEC if rule == "spec" else _lib.SD_RULE_ENGINE
        assert len(self.trows) == self.g + (1 if rule == "spec" else 0)
        self.spec = ops.ProcSpec("multinomial", 1.0)
        self.draft = torch.zeros(self.B, self.g, dtype=torch.long, device=DEV)
        self.stats = torch.empty(self.g, self.B, 2, device=DEV)
        self.counts = torch.zeros(self.B, 2, dtype=torch.long, device=DEV) if counts else None
        self.state = None
        if engine:
            self.state = dict(generated=torch.zeros(self.B, 3 * self.g, dtype=torch.long, device=DEV), step=self.g,
                              finished=torch.zeros(self.B, dtype=torch.uint8, device=DEV),
                              accepted=torch.zeros(self.B, dtype=torch.long, device=DEV))
        self.active = active
        self.override = draft_override   # (mask [B, g] bool, tokens [B, g]) applied after the draws
        self.stop = stop if stop is not None else torch.tensor([3], device=DEV)

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()
        if self.state is not None:
            for k in ("generated", "finished", "accepted"):
                self.state[k].zero_()

    def __call__(self, noise):
        from specdec_amd import ops
        for d in range(self.g):
            ops.sample_rows(self.drows[d], self.spec, noise, tokens_out=self.draft[:, d], row_stats_out=self.stats[d])
        if self.override is not None:
            self.draft.copy_(torch.where(self.override[0], self.override[1], self.draft))
        extra = {}
        if self.rule != 0:
            extra = dict(engine_state=self.state, active=self.active)
        return ops.verify(self.trows, self.drows, self.draft, self.rule, self.spec, self.spec, noise, self.stop,
                          draft_row_stats=self.stats, row_counts=self.counts, **extra)

    def snapshot(self, out):
        torch.cuda.synchronize()
        res = {k: getattr(out, k).cpu().clone() for k in OUT_FIELDS}
        res["draft"] = self.draft.cpu().clone()
        if self.counts is not None:
            res["counts"] = self.counts.cpu().clone()
        if self.state is not None:
            res.update({k: v.cpu().clone() for k, v in self.state.items() if torch.is_tensor(v)})
        return res


def once(step, kind, seed, want=None, **kw):
    """One eager step on `kind`'s path from a reset state; asserts the path taken."""
    from specdec_amd import PhiloxNoise, _lib
    step.reset()
    with path(kind, **kw):
        res = step.snapshot(step(PhiloxNoise(seed=seed)))
    got = _lib.last_verify_path()
    if want is None:
        want = _lib.SD_PATH_VERIFY_FUSED if kind == "fused" else _lib.SD_PATH_VERIFY_TWO_LAUNCH
    assert got == want, _lib.PATH_NAMES.get(got)
    return res


def check_decided(res, rule, B):
    from specdec_amd import _lib
    assert (res["row_status"] & _lib.SD_ROW_DONE).all()
    assert not (res["row_status"] & _lib.SD_ROW_ERROR_MASK).any()


def rows_of(tl, dl, rule):
    g = dl.shape[1]
    return [tl[:, t] for t in range(g + (1 if rule == "spec" else 0))], [dl[:, d] for d in range(g)]


# ---------------------------------------------------------------- two-chunk sampler edges
EDGE_V = [2048, 2056, 4096, 4104, 6152, 10248]   # chunks: 1 | 1 + 8 el. | 2 | 2 + 8 el. | 3 + 8 el. (even) | 5 + 8 el.
# 2056 and 4104 leave a chunk of 8 elements (as a sampler's second chunk, and alone in the last sampler);
# 4104 has an odd chunk count (the last sampler draws one chunk); every V but 2048 / 4096 ends on a ragged chunk.


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("B", [8, 16])
def test_two_chunk_sampler_edges(B, g, dt, rule):
    for V in EDGE_V:
        seed = 7 * B + 3 * g + V % 97 + (1 if dt == "fp16" else 0) + (50 if rule == "spec" else 0)
        tl, dl = logits(B, g, V, dt, seed)
        # odd rows reject draft b % g (its id is the drafter's likeliest token, without mass under the
        # target), so residual rows are drawn whatever the other rows' walks do
        mask = torch.zeros(B, g, dtype=torch.bool, device=DEV)
        tok = torch.zeros(B, g, dtype=torch.long, device=DEV)
        for b in range(1, B, 2):
            i = b % g
            k = int(dl[b, i].float().argmax())
            dl[b, i, k] += 12.0
            tl[b, i, k] = -100.0
            mask[b, i], tok[b, i] = True, k
        step = Step(*rows_of(tl, dl, rule), rule, engine=rule == "engine", draft_override=(mask, tok))
        two = once(step, "two", seed)
        got = once(step, "fused", seed)
        assert_same(got, two, (V,))
        check_decided(two, rule, B)
        # the branch under test is reached: the odd rows drew a residual token
        from specdec_amd import _lib
        odd = slice(1, B, 2)
        assert (two["row_status"][odd] & _lib.SD_ROW_RESIDUAL).all()
        assert ((two["next_token"][odd] >= 0) & (two["next_token"][odd] < V)).all()


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("case", ["misaligned", "fp32"])
def test_misaligned_and_fp32_rows(case, rule):
    """A row base shifted by one element (the samplers' one-chunk-at-a-time path) and fp32 rows (two
    vectors per thread and chunk: the general path): untouched code, the same outputs."""
    B, g = 8, 4
    if case == "fp32":
        V = 6149
        tl, dl = logits(B, g, V, "fp32", 11)
    else:
        V = 6152
        tw, dw = logits(B, g, V + 8, "bf16", 12)
        tl, dl = tw[:, :, 1:V + 1], dw[:, :, 1:V + 1]
        assert tl[:, 0].data_ptr() % 16 == 2 and dl[:, 0].data_ptr() % 16 == 2
    step = Step(*rows_of(tl, dl, rule), rule, engine=rule == "engine")
    two = once(step, "two", 21)
    assert_same(once(step, "fused", 21), two)
    check_decided(two, rule, B)


# ---------------------------------------------------------------- nothing to sample / fallback row
def test_rows_without_sampling_beside_sampling_rows_and_a_fallback_row():
    """ENGINE rule, B = 8, gamma = 4, V = 6152 (four chunks, the last of 8 elements).
    rows 0, 1: drafter rows equal the target rows -> every draft accepted, nothing to sample (mode none);
    row 2: rejected at draft 0, row 3: rejected at draft gamma - 1 (the drafted id is the drafter's
      likeliest token, which the target gives no mass) -> residual rows next to the empty ones;
    row 4: target and drafter rows of slot 0 hold four tokens of mass and nothing else (logit -100: a
      probability of exactly 0); the rows are equal except at the drafted id, which the drafter gives
      ~1e-27 and the target 0.  p / q = 0 rejects it, the residual (p - q)+ sums to 0 <= 1e-12 and the
      engine samples the target row itself (SD_ROW_FALLBACK_P);
    rows 5 .. 7: random rows.
    The two-launch outputs are checked to have taken these branches before the fused ones are compared."""
    from specdec_amd import _lib
    B, g, V = 8, 4, 6152
    tl, dl = logits(B, g, V, "bf16", 33)
    tl = tl[:, :g].contiguous()
    dl[0:2] = tl[0:2]
    mask = torch.zeros(B, g, dtype=torch.bool, device=DEV)
    tok = torch.zeros(B, g, dtype=torch.long, device=DEV)
    for b, i in ((2, 0), (3, g - 1)):
        dl[b, :i] = tl[b, :i]                      # accepted up to draft i
        k = int(dl[b, i].float().argmax())
        dl[b, i, k] += 12.0                        # q(k) ~ 1
        tl[b, i, k] = -100.0                       # p(k) = 0
        mask[b, i], tok[b, i] = True, k
    heavy = torch.tensor([5, 2047, 2048, 6151], device=DEV)   # first / last lanes of chunks 0 and 1, the last element
    tl[4, 0] = -100.0
    tl[4, 0, heavy] = torch.tensor([2.0, 1.0, 0.5, 0.0], device=DEV).to(tl.dtype)
    dl[4, 0] = tl[4, 0]
    kf = 4100                                      # the drafted id of row 4: chunk 2
    dl[4, 0, kf] = -60.0
    mask[4, 0], tok[4, 0] = True, kf
    step = Step(*rows_of(tl, dl, "engine"), "engine", engine=True, draft_override=(mask, tok))
    two = once(step, "two", 44)
    n, st = two["n_accepted"], two["row_status"]
    assert n[0] == g and n[1] == g and not (st[0:2] & (_lib.SD_ROW_RESIDUAL | _lib.SD_ROW_FALLBACK_P)).any()
    assert (two["next_token"][0:2] == -1).all()    # nothing sampled
    assert n[2] == 0 and n[3] == g - 1 and (st[2:4] & _lib.SD_ROW_RESIDUAL).all()
    assert n[4] == 0 and (st[4] & _lib.SD_ROW_FALLBACK_P) and not (st[4] & _lib.SD_ROW_RESIDUAL)
    assert float(two["resample_mass"][4]) <= 1e-12
    assert int(two["next_token"][4]) in heavy.tolist()
    check_decided(two, "engine", B)
    assert_same(once(step, "fused", 44), two)
    # and with the empty rows inactive (rows the engine leaves alone)
    step.active = torch.tensor([0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    two = once(step, "two", 45)
    assert not (two["row_status"][[0, 5]] & _lib.SD_ROW_DONE).any()
    assert_same(once(step, "fused", 45), two)


# ---------------------------------------------------------------- row_counts
def emitted(res):
    """(accepted drafts, tokens emitted) of one call's rows, from its outputs."""
    from specdec_amd import _lib
    done = (res["row_status"] & _lib.SD_ROW_DONE) != 0
    n = torch.where(done, res["n_accepted"].long(), torch.zeros_like(res["n_accepted"].long()))
    return torch.stack([n, n + (done & (res["next_token"] >= 0)).long()], dim=1)


def three_eager(step, kind, seed):
    from specdec_amd import PhiloxNoise, _lib
    step.reset()
    noise = PhiloxNoise(seed=seed)
    snaps = []
    with path(kind):
        for _ in range(3):
            snaps.append(step.snapshot(step(noise)))
            want = _lib.SD_PATH_VERIFY_FUSED if kind == "fused" else _lib.SD_PATH_VERIFY_TWO_LAUNCH
            assert _lib.last_verify_path() == want
    return snaps


def three_replays(step, seed):
    """One step (its draws, the verify, the device noise offset's advance) captured once, replayed three
    times on the eager calls' workspace: the replays draw what three consecutive eager calls draw."""
    from specdec_amd import PhiloxNoise, _lib
    off = torch.zeros(1, dtype=torch.long, device=DEV)
    calls = step.g + 1
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with path("fused"), torch.cuda.stream(stream):
        step(PhiloxNoise(seed=seed, offset_dev=off))   # warm-up (allocations)
        noise = PhiloxNoise(seed=seed, offset_dev=off)
        with torch.cuda.graph(graph, stream=stream):
            out = step(noise)
            noise.advance_device(calls)
        assert _lib.last_verify_path() == _lib.SD_PATH_VERIFY_FUSED
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    step.reset()
    off.zero_()
    snaps = []
    for _ in range(3):
        graph.replay()
        snaps.append(step.snapshot(out))
    return snaps


@pytest.mark.parametrize("mode", ["spec", "engine", "engine-state"])
@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no-counts"])
def test_row_counts_accumulate_over_calls_and_replays(mode, counts):
    B, g, V = 8, 4, 6152
    rule = "spec" if mode == "spec" else "engine"
    tl, dl = logits(B, g, V, "bf16", 55)
    active = (torch.arange(B, device=DEV) % 5 != 3).to(torch.uint8) if rule == "engine" else None
    step = Step(*rows_of(tl, dl, rule), rule, engine=mode == "engine-state", active=active, counts=counts)
    two = three_eager(step, "two", 66)
    runs = {"eager": three_eager(step, "fused", 66), "graph": three_replays(step, 66)}
    for name, snaps in runs.items():
        total = torch.zeros(B, 2, dtype=torch.long)
        for i in range(3):
            assert_same(snaps[i], two[i], (name, i))
            total += emitted(snaps[i])
            if counts:
                assert torch.equal(snaps[i]["counts"], total), (name, i)
        assert total[:, 1].sum() > total[:, 0].sum() > 0   # drafts were accepted and tokens sampled
    assert not torch.equal(two[0]["next_token"], two[1]["next_token"])   # the calls drew fresh noise


# ---------------------------------------------------------------- row layouts
def laid_out(x, way):
    """The rows [B, V] of x [B, T, V] in one of the layouts the launcher tells apart."""
    B, T, V = x.shape
    if way == "views":      # x[:, t, :] of one tensor: equally spaced, the kernel forms the addresses from parameters
        return [x[:, t] for t in range(T)]
    if way == "separate":   # separately allocated, neither ascending nor equally spaced: the row-pointer table
        pool = sorted((torch.empty(B, V, dtype=x.dtype, device=DEV) for _ in range(T + 2)), key=lambda t: t.data_ptr())
        order = ([pool[1], pool[0]] + pool[3:] + [pool[2]])[:T]
        for t in range(T):
            order[t].copy_(x[:, t])
        return order
    assert way == "alias"   # one tensor shared by every slot: stride 0
    one = x[:, 0].contiguous()
    return [one] * T


@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("B,g", [(8, 4), (16, 1)])
def test_row_layouts(B, g, rule):
    V = 4104
    tl, dl = logits(B, g, V, "bf16", 77 + B)
    n_t = g + (1 if rule == "spec" else 0)
    ref = None
    for way in ("views", "separate", "alias"):
        step = Step(laid_out(tl[:, :n_t], way), laid_out(dl, way), rule, engine=rule == "engine")
        two = once(step, "two", 88)
        check_decided(two, rule, B)
        for fast in (1, 0):
            assert_same(once(step, "fused", 88, arg_fast=fast), two, (way, fast))
        if way != "alias":   # the same logits, however the rows are laid out
            ref = ref or two
            assert_same(two, ref, way)


# ---------------------------------------------------------------- forced ticket order
@pytest.mark.parametrize("rule", ["engine", "spec"])
@pytest.mark.parametrize("sc", [2, 4])
@pytest.mark.parametrize("B", [8, 32])
def test_forced_ticket_order(B, sc, rule):
    from specdec_amd import _lib
    g, V = 4, 10248
    tl, dl = logits(B, g, V, "bf16", 99 + B)
    step = Step(*rows_of(tl, dl, rule), rule, engine=rule == "engine")
    two = once(step, "two", 111)
    got = once(step, "fused", 111, want=_lib.SD_PATH_VERIFY_FUSED_TICKET, ticket=1, samp_chunks=sc)
    assert_same(got, two)
    check_decided(two, rule, B)
