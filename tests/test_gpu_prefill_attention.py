"""GPU tests of sd_prefill_attention (ops.prefill_attention, csrc/prefill_attention.hip) against the fp64 reference of
tests/test_gpu_tree_attention_ragged.py over the visible keys, visible[b, r, j] = r < n_b and j <= len_b - n_b + r.
Every position at or beyond len_b, every unused page and every slot past the length holds NaN (FP8: the NaN byte),
so a kernel that reads one of them into the result fails the finiteness check.

Tolerance (unchanged): 2 eps max|V| over the visible keys; FP8: V = v_scale * e4m3 value."""
import pytest
import torch

from test_gpu_tree_attention_paged import _bytes, _dev, _places, _pool, _quantised
from test_gpu_tree_attention_ragged import BAD, BF, DEV, HF, _long, _reference

pytestmark = pytest.mark.gpu

G1 = (BF, 64, 2, 2, 130, ((130, 130), (200, 129), (64, 1), (0, 0)))     # Rb = 128: two blocks, a one-row block, empty
G4 = (HF, 128, 8, 2, 70, ((70, 70), (333, 65), (97, 33), (5, 5)))       # Rb = 32: the diagonal mid-tile, odd prefix
G8 = (BF, 128, 8, 1, 40, ((40, 40), (129, 17), (64, 16), (65, 40)))     # Rb = 16: two heads a wave tile, tile borders
G3 = (HF, 64, 6, 2, 33, ((33, 33), (128, 32), (192, 1)))
G2 = (BF, 64, 2, 1, 70, ((16500, 70), (16449, 3)))                      # Rb = 64; S = 16: a second window of page ids
# (shape, FP8, page size or None, lengths as a tensor plus this addend and rows as an int)
CASES = [(G1, False, None, 0), (G4, False, None, 0), (G8, False, None, 0), (G3, False, None, 0),
         (G4, True, None, 0), (G8, True, None, 0),
         (G4, True, 16, 0), (G4, False, 128, 0), (G8, False, 16, 0), (G8, True, 128, 0), (G2, False, 16, 0),
         ((HF, 128, 4, 1, 33, ((33, 33), (100, 33), (64, 33))), False, None, 7)]


def _case(shape, fp8=False, seed=0):
    """(q, k, v, scales, dequantised k, v, visible) on the CPU; positions at or beyond len_b hold NaN."""
    dtype, D, Hq, Hkv, R, seqs = shape
    gen = torch.Generator().manual_seed(seed)
    B, L = len(seqs), max(s[0] for s in seqs) + 9
    lens, ns = (torch.tensor([s[i] for s in seqs]) for i in (0, 1))
    q = torch.randn(B, R, Hq, D, generator=gen).to(dtype).transpose(1, 2)
    k, v = (torch.randn(B, Hkv, L, D, generator=gen).to(dtype) for _ in range(2))
    j, r = torch.arange(L), torch.arange(R)
    for t in (k, v):
        t[(j >= lens[:, None])[:, None, :].expand(B, Hkv, L)] = float("nan")
    visible = (r[None, :, None] < ns[:, None, None]) & (j[None, None, :] <= (lens - ns)[:, None, None] + r[None, :, None])
    scales, kr, vr = {}, k, v
    if fp8:
        k, v, ks, vs, kr, vr = _quantised(k, v, Hkv)
        scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    return q, k, v, scales, kr, vr, visible


def _run(q, k, v, lens, ns, S=None, place=None, num_pages=None, **kw):
    from specdec_amd import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    if S is None:
        out = ops.prefill_attention(q.to(DEV), _dev(k), _dev(v), lens, rows=ns, status_or=status, **kw)
    else:
        host_lens = kw.pop("host_lens")                       # the permuted [P, S, Hkv, D] pool
        (kp, table), (vp, _) = (_pool(t, host_lens, S, place, num_pages, True) for t in (k, v))
        out = ops.prefill_attention(q.to(DEV), _dev(kp), _dev(vp), lens, rows=ns, status_or=status, block_table=table.to(DEV), **kw)
    return out, int(status.item())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"G{c[0][2] // c[0][3]}-D{c[0][1]}-R{c[0][4]}-fp8{int(c[1])}-S{c[2]}-add{c[3]}")
def test_prefill_matches_the_fp64_reference(case):
    shape, fp8, S, add = case
    dtype, D, Hq, Hkv, R, seqs = shape
    q, k, v, scales, kr, vr, visible = _case(shape, fp8)
    want = _reference(q, kr, vr, visible, D ** -0.5)
    host_lens, host_ns = [s[0] for s in seqs], [s[1] for s in seqs]
    lens, ns = _long(host_lens, add), (host_ns[0] if add else _long(host_ns))
    kw = dict(kv_len_add=add, kv_cap=max(host_lens), **scales)
    out, status = _run(q, k, v, lens, ns, **kw)
    got = out.cpu().double()
    seen = visible.any(1)[:, None, :, None].expand(len(seqs), Hkv, k.shape[2], D)
    tol = 2 * torch.finfo(dtype).eps * float(vr[seen].double().abs().max())
    err = float((got - want).abs().max())
    print(f"[prefill-attn] {case}: max err {err:.3g}, tol {tol:.3g}")
    assert out.shape == (len(seqs), R, Hq, D) and out.dtype == dtype and status == 0
    assert torch.isfinite(got).all()
    assert err <= tol
    for b, (_, n) in enumerate(seqs):                         # padding rows and empty sequences: exact zeros
        assert not got[b, n:].any(), b
    if S is not None:                                         # the same arithmetic at other addresses
        ident, perm, num_pages = _places(len(seqs), -(-k.shape[2] // S), seed=R)
        for place in (perm, ident):
            paged, status = _run(q, k, v, lens, ns, S, place, num_pages, host_lens=host_lens, **kw)
            assert status == 0 and torch.equal(_bytes(paged), _bytes(out))


def test_a_sequence_does_not_depend_on_the_rest_of_the_batch():
    _, _, _, _, _, seqs = G4
    q, k, v, _, _, _, _ = _case(G4, seed=2)
    batch, _ = _run(q, k, v, _long([s[0] for s in seqs]), _long([s[1] for s in seqs]), kv_cap=333)
    for b, (length, n) in enumerate(seqs):
        s = slice(b, b + 1)
        alone, _ = _run(q[s], k[s], v[s], _long([length]), _long([n]), kv_cap=333)
        assert torch.equal(_bytes(alone), _bytes(batch[s])), b


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_a_captured_call_follows_lengths_rows_and_table_rows_written_in_place(paged):
    from specdec_amd import ops
    dtype, D, Hq, Hkv, R, _ = G4
    steps, S = [((70, 40), (70, 7)), ((333, 200), (65, 70))], 16             # (lengths, rows)
    q, k, v, _, _, _, _ = _case((dtype, D, Hq, Hkv, R, ((333, 0), (333, 0))), seed=4)
    kw, tables = {}, None
    if paged:
        _, perm, num_pages = _places(2, -(-k.shape[2] // S), seed=7)
        (k, t0), (v, _) = (_pool(t, (333, 333), S, perm, num_pages) for t in (k, v))
        tables = (t0, t0.flip(0).contiguous())                # the sequences trade their pages
        kw = dict(block_table=t0.to(DEV))
    q, k, v = q.to(DEV), _dev(k), _dev(v)
    kv_len, rows = _long(steps[0][0]), _long(steps[0][1])
    out = torch.empty(2, R, Hq, D, dtype=dtype, device=DEV)
    call = lambda o=None: ops.prefill_attention(q, k, v, kv_len, rows=rows, kv_cap=333, out=o, **kw)
    graph = None
    for i, (lens, ns) in enumerate(steps):
        kv_len.copy_(_long(lens)), rows.copy_(_long(ns))
        if paged:
            kw["block_table"].copy_(tables[i % 2])
        eager = call()
        if graph is None:                                     # captured on the first step's values only
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call(out)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert eager.float().abs().sum() > 0
        assert torch.equal(_bytes(out), _bytes(eager)), i


def test_clamped_lengths_and_rows_are_flagged():
    _, _, _, _, _, seqs = G4
    q, k, v, _, _, _, _ = _case(G4, seed=5)
    k, v = k.nan_to_num(0.5), v.nan_to_num(0.25)
    lens, ns = [s[0] for s in seqs], [s[1] for s in seqs]
    clean, status = _run(q, k, v, _long(lens), _long(ns), kv_cap=333)
    assert status == 0
    over, status = _run(q, k, v, _long([lens[0], 500] + lens[2:]), _long(ns), kv_cap=333)     # a length above kv_cap
    assert status == BAD and torch.equal(_bytes(over), _bytes(clean))
    many, status = _run(q, k, v, _long(lens), _long(ns[:3] + [9]), kv_cap=333)                # rows_dev[3] above len_3 = 5
    assert status == BAD and torch.equal(_bytes(many), _bytes(clean))


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("bad_id", [-1, "num_pages"])
def test_a_page_id_out_of_range_is_refused(fp8, bad_id):
    from specdec_amd import ops
    dtype, D, Hq, Hkv, R, seqs = G4
    S, lens, ns = 16, [s[0] for s in seqs], [s[1] for s in seqs]
    q, k, v, scales, _, _, _ = _case(G4, fp8, seed=6)
    _, perm, num_pages = _places(len(seqs), -(-k.shape[2] // S), seed=1)
    (kp, table), (vp, _) = (_pool(t, lens, S, perm, num_pages) for t in (k, v))
    kp, vp = _dev(kp), _dev(vp)
    kp0, vp0 = kp.clone(), vp.clone()
    kw = dict(rows=_long(ns), kv_cap=333, **scales)
    clean = ops.prefill_attention(q.to(DEV), kp, vp, _long(lens), block_table=table.to(DEV), **kw)
    table[1, 3] = num_pages if bad_id == "num_pages" else bad_id     # keys 48..63 of sequence 1: inside its length
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.prefill_attention(q.to(DEV), kp, vp, _long(lens), block_table=table.to(DEV), status_or=status, **kw)
    assert int(status.item()) == BAD
    assert torch.isfinite(out[1].float()).all()
    assert torch.equal(_bytes(out[[0, 2, 3]]), _bytes(clean[[0, 2, 3]]))
    assert torch.equal(_bytes(kp), _bytes(kp0)) and torch.equal(_bytes(vp), _bytes(vp0))


def test_a_prompt_forward_through_a_model():
    """The bf16 test Llama, a 150-token prompt under tree_attention.causal against the stock sdpa forward, held to
    that file's yardstick: 4 x the stock sdpa-vs-eager difference on the same forward."""
    pytest.importorskip("transformers")
    from specdec_amd import tree_attention
    from test_gpu_tree_attention_model import _bound, _llama
    model = _llama(1)
    tokens = torch.randint(0, 512, (1, 150), generator=torch.Generator().manual_seed(8)).to(DEV)

    def forward(stock):
        model.config._attn_implementation = stock
        with torch.no_grad():
            return model(input_ids=tokens, use_cache=True).logits[0]

    eager, sdpa = forward("eager"), forward("sdpa")
    before = tree_attention.counts["kernel"]
    with tree_attention.causal(model, 150, DEV):
        got = forward(model.config._attn_implementation)
    assert tree_attention.counts["kernel"] == before + model.config.num_hidden_layers
    diff, bound = float((got.float() - sdpa.float()).abs().max()), _bound(sdpa, eager, eager)
    print(f"[prefill-attn] model: kernel vs sdpa {diff:.3g}, bound {bound:.3g}")
    assert torch.isfinite(got).all() and diff <= bound
