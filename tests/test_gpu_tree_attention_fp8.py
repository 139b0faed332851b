"""GPU tests of tree attention over an FP8 KV cache (sd_tree_attention_fp8 / sd_tree_attention_ragged_fp8 through
ops.tree_attention, csrc/tattn_fp8_tile.inc) against fp64 attention on ``fp8 value * scale``, in the scheme of
tests/test_gpu_tree_attention.py: inputs built on the CPU, K/V slices of a longer buffer, and every position no
row of its sequence sees, or at or beyond the length, holding the e4m3 NaN byte.  The scales differ per head and
are no powers of two, so a wrong head index shows.

Tolerance: DESIGN.md §4i's 2 eps max|V| unchanged, V = v_scale * fp8 over the visible keys: every e4m3 value is
exactly a bf16 and an fp16 value, and the scales multiply fp32 numbers outside the matrix products."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn

# (q dtype, D, Hq, Hkv, R, kv_len, splits, win_base, B, q transposed, reach: the largest kv_limit)
CASES = [
    (BF, 64, 2, 2, 1, 1, 0, 0, 1, False, None),               # one key, one row
    (HF, 128, 4, 1, 29, 63, 0, 0, 1, False, None),            # a partial tile, a group of 4 on one K/V stream
    (BF, 128, 8, 2, 33, 64, 0, 61, 1, True, None),            # two row tiles, the window cut off by kv_len
    (BF, 64, 4, 1, 128, 333, 1, 77, 1, False, None),          # 512 query rows: four passes
    (HF, 128, 2, 2, 29, 333, 5, 77, 3, False, None),          # five splits through the combine, the last tile partial
    (BF, 128, 4, 1, 29, 333, 5, 77, 1, False, 100),           # splits no row reaches
]


def _scales(Hkv):
    h = torch.arange(Hkv, dtype=torch.float32)
    return 0.5 + 0.37 * h, 1.25 - 0.11 * h


def _case(dtype, D, Hq, Hkv, R, L, win_base, B, transposed, reach, lens=None, seed=0):
    """(q, k, v, kv_limit, win_bits, visible [B, R, L + 9]) on the CPU; lens: per-sequence lengths (default L)."""
    gen = torch.Generator().manual_seed(seed)
    A = L + 9
    q = torch.randn(B, R, Hq, D, generator=gen).to(dtype)
    q = q.transpose(1, 2) if transposed else q.transpose(1, 2).contiguous()
    kbuf, vbuf = (torch.randn(B, Hkv, A + 8, D, generator=gen).to(F8) for _ in range(2))
    limit = torch.randint(0, (reach or L) + 1, (B, R), generator=gen)
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, R), generator=gen, dtype=torch.int64)
    if R >= 5:
        limit[:, 0], bits[:, 1] = 0, -1                       # a row of window keys only; all 64 bits
        limit[:, 2] = min(L, win_base + 5)
        bits[:, 3] = 0
        limit[:, 4], bits[:, 4] = 0, 0                        # nothing visible: zeros
    else:
        limit[:, 0].clamp_(min=1)
    lens = torch.full((B,), L) if lens is None else torch.tensor(lens)
    j = torch.arange(A)
    rel = (j - win_base).clamp(0, 63)
    in_win = ((bits[:, :, None] >> rel) & 1).bool() & (j >= win_base) & (j < win_base + 64)
    visible = ((j < limit[:, :, None]) | in_win) & (j < lens[:, None, None])
    dead = ~visible.any(1)
    for buf in (kbuf, vbuf):
        buf.view(torch.uint8)[:, :, 5:5 + A][dead[:, None, :].expand(B, Hkv, A)] = 0x7F     # the NaN byte
    return q, kbuf[:, :, 5:5 + A], vbuf[:, :, 5:5 + A], limit.int(), bits, visible


def _reference(q, k, v, ks, vs, visible, scale):
    G = q.shape[1] // k.shape[1]
    kd = (k.double().nan_to_num(0.0) * ks.double()[None, :, None, None]).repeat_interleave(G, 1)
    vd = (v.double().nan_to_num(0.0) * vs.double()[None, :, None, None]).repeat_interleave(G, 1)
    s = (q.double() @ kd.transpose(2, 3)) * scale
    p = s.masked_fill(~visible[:, None], float("-inf")).softmax(-1).nan_to_num(0.0)
    return (p @ vd).transpose(1, 2), vd


def _to_dev(q, k, v, transposed=False):
    qd = q.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) if transposed else q.to(DEV)
    kd, vd = (torch.empty_strided(t.shape, t.stride(), dtype=torch.uint8, device=DEV).copy_(t.view(torch.uint8)).view(F8)
              for t in (k, v))
    return qd, kd, vd


def _check(tag, out, q, k, v, ks, vs, visible, dtype, R):
    want, vd = _reference(q, k, v, ks, vs, visible, q.shape[3] ** -0.5)
    got = out.cpu().double()
    seen = visible.any(1)[:, None, :, None].expand_as(vd)
    tol = 2 * torch.finfo(dtype).eps * float(vd[seen].abs().max())
    err = float((got - want).abs().max())
    print(f"[tree-attn-fp8] {tag}: max err {err:.3g}, tol {tol:.3g}")
    assert torch.isfinite(got).all()
    assert err <= tol
    if R >= 5:
        assert not got[:, 4].any()                            # the row that sees nothing
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_fp8_tree_attention_matches_the_fp64_reference(case):
    from specdec_amd import ops
    dtype, D, Hq, Hkv, R, kv_len, splits, win_base, B, transposed, reach = case
    q, k, v, limit, bits, visible = _case(dtype, D, Hq, Hkv, R, kv_len, win_base, B, transposed, reach)
    ks, vs = _scales(Hkv)
    qd, kd, vd = _to_dev(q, k, v, transposed)
    out = ops.tree_attention(qd, kd, vd, limit.to(DEV), bits.to(DEV), win_base, kv_len=kv_len, splits=splits,
                             k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    assert out.shape == (B, R, Hq, D) and out.dtype == dtype
    _check(case, out, q, k, v, ks, vs, visible, dtype, R)


LENS = (0, 65, 333)


@pytest.mark.parametrize("chunk_tiles", [2, 0])
@pytest.mark.parametrize("dtype, D", [(BF, 64), (HF, 128), (BF, 128), (HF, 64)])
def test_ragged_fp8_matches_the_reference_and_each_sequence_alone(dtype, D, chunk_tiles):
    """Lengths (0, 65, 333) under kv_cap 333 with a device win_base: chunk slots beyond a sequence's length, the
    zeros of a length-0 sequence; and every sequence's output bit-identical alone and inside the batch."""
    from specdec_amd import ops
    Hq, Hkv, R, B = 4, 2, 29, 3
    q, k, v, limit, bits, visible = _case(dtype, D, Hq, Hkv, R, 333, 0, B, False, None, lens=LENS)
    # per-sequence window bases: rebuild the visibility of the window part under them
    bases = torch.tensor([0, 40, 300])
    j = torch.arange(k.shape[2])
    rel = (j[None] - bases[:, None]).clamp(0, 63)[:, None, :]
    in_win = ((bits[:, :, None] >> rel) & 1).bool() & (j[None, None] >= bases[:, None, None]) & (j[None, None] < bases[:, None, None] + 64)
    lens = torch.tensor(LENS)
    visible = ((j < limit[:, :, None]) | in_win) & (j < lens[:, None, None])
    for buf in (k, v):                                        # what is dead under these bases holds NaN; the rest is finite
        raw = buf.view(torch.uint8)
        raw[raw == 0x7F] = 0x30
        raw[(~visible.any(1))[:, None, :].expand(B, Hkv, -1)] = 0x7F
    ks, vs = _scales(Hkv)
    qd, kd, vd = _to_dev(q, k, v)
    args = dict(kv_cap=333, chunk_tiles=chunk_tiles, k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    out = ops.tree_attention(qd, kd, vd, limit.to(DEV), bits.to(DEV), bases.to(DEV), kv_len=lens.to(DEV), **args)
    got = _check((dtype, D, chunk_tiles), out, q, k, v, ks, vs, visible, dtype, R)
    assert not got[0].any()                                   # the sequence of length 0
    for b in range(B):
        alone = ops.tree_attention(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], limit[b:b + 1].to(DEV), bits[b:b + 1].to(DEV),
                                   bases[b:b + 1].to(DEV), kv_len=lens[b:b + 1].to(DEV), **args)
        assert torch.equal(alone.view(torch.int16), out[b:b + 1].view(torch.int16))


def test_a_captured_fp8_call_follows_scales_and_lengths_overwritten_in_place():
    from specdec_amd import ops
    q, k, v, limit, bits, _ = _case(BF, 128, 4, 2, 29, 333, 0, 2, False, None, seed=3)
    for buf in (k, v):
        buf.view(torch.uint8)[buf.view(torch.uint8) == 0x7F] = 0x30     # every length below sees finite values
    qd, kd, vd = _to_dev(q, k, v)
    limit, bits = limit.to(DEV), bits.to(DEV)
    base = torch.tensor([77, 200], device=DEV)
    lens = torch.tensor([333, 100], device=DEV)
    ks, vs = (t.to(DEV) for t in _scales(2))
    call = lambda out=None: ops.tree_attention(qd, kd, vd, limit, bits, base, kv_len=lens, kv_cap=333, chunk_tiles=2,
                                               out=out, k_scale=ks, v_scale=vs)
    out = torch.empty_like(call())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out)
    for new_lens, mul in (((333, 100), 1.0), ((64, 333), 1.7), ((200, 1), 0.3)):
        lens.copy_(torch.tensor(new_lens))
        ks.mul_(mul)
        vs.mul_(mul)
        eager = call()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))


@pytest.mark.parametrize("change, error", [
    (dict(no_scales=True), ValueError), (dict(kv16=True), ValueError),
    (dict(dtype=torch.float32), -4), (dict(D=96), -4), (dict(R=129), -4), (dict(short_workspace=True), -2)])
def test_fp8_argument_errors(change, error):
    """Missing scales, scales with 16-bit K/V: ValueError.  fp32 q, D = 96 and R = 129: SD_ERR_UNSUPPORTED; a
    workspace one byte short: SD_ERR_WORKSPACE."""
    from specdec_amd import _lib, ops
    c = dict(dtype=BF, D=64, Hq=4, Hkv=2, R=8, short_workspace=False, no_scales=False, kv16=False)
    c.update(change)
    q = torch.zeros(1, c["Hq"], c["R"], c["D"], dtype=c["dtype"], device=DEV)
    k = torch.zeros(1, c["Hkv"], 333, c["D"], dtype=torch.uint8, device=DEV).view(F8)
    if c["kv16"]:
        k = k.to(c["dtype"])
    limit = torch.zeros(1, c["R"], dtype=torch.int32, device=DEV)
    s = None if c["no_scales"] else torch.ones(c["Hkv"], device=DEV)
    ws = None
    if c["short_workspace"]:
        need = _lib.lib.sd_tree_attention_workspace_size(1, c["Hq"], c["Hkv"], c["R"], c["D"], 333, 2)
        ws = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    expect = pytest.raises(ValueError) if error is ValueError else pytest.raises(_lib.SpecdecError, match=rf"\({error}\)")
    with expect:
        ops.tree_attention(q, k, k, limit, limit.long(), 0, splits=2, workspace=ws, k_scale=s, v_scale=s)
