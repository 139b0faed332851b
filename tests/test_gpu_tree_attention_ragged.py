"""GPU tests of sd_tree_attention_ragged (ops.tree_attention with device tensors for kv_len / win_base,
csrc/tree_attention.hip) against an fp64 torch reference computed on the CPU from the same 16-bit inputs
with a per-sequence visibility mask.  Every K/V position that no row of its sequence sees, and every
position at or beyond the sequence's own length — [len_b, kv_cap) and [kv_cap, L) — holds NaN, so a kernel
that reads one of them into the result fails the finiteness check.

Tolerance (unchanged): 2 eps max|V| over the visible keys of the case."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16
BAD = 0x40                                                    # SD_ROW_INVALID_DIST

# (dtype, D, Hq, Hkv, R, lengths, kv_cap, chunk_tiles, win_base: an int for the batch or one per sequence,
#  (kv_len_add, win_base_add))
CASES = [
    (BF, 64, 2, 2, 1, (1, 64, 333), 333, 1, (0, 60, 300), (0, 0)),          # 1, 1 and 6 chunks, the last tile partial
    (HF, 128, 4, 1, 29, (1, 64, 333), 333, 1, (0, 3, 330), (0, 0)),
    (BF, 64, 8, 2, 128, (1, 64, 333), 333, 1, (0, 60, 300), (0, 0)),        # 512 query rows: four passes
    (BF, 128, 8, 2, 65, (0, 333, 65), 400, 2, 50, (0, 0)),                  # an empty sequence; slots beyond every length
    (HF, 64, 2, 2, 29, (0, 333, 65), 400, 2, 0, (0, 0)),
    (BF, 64, 4, 1, 128, (128, 129, 127), 333, 2, 100, (0, 0)),              # on, one past, one short of a chunk border
    (HF, 128, 2, 2, 1, (128, 129, 127), 333, 2, 120, (0, 0)),
    (BF, 128, 4, 1, 29, (40, 64), 64, 0, 30, (0, 0)),                       # C == 1: written directly, no workspace
    (HF, 64, 8, 2, 65, (40, 64), 64, 0, 0, (0, 0)),
    (BF, 128, 8, 2, 65, (333, 100, 7, 200), 333, 0, (330, 97, 0, 190), (0, 0)),   # windows cut off by len_b; the auto rule
    (HF, 64, 4, 4, 29, (333, 100, 7, 200), 333, 0, (330, 97, 0, 190), (0, 0)),
    (BF, 128, 4, 1, 29, (229,), 333, 0, (201,), (29, 1)),                   # one cumulative_length-style tensor, addends
]


def _case(dtype, D, Hq, Hkv, R, lens, kv_cap, win_base, seed=0):
    """(q, k, v, kv_limit, win_bits, visible [B, R, L] bool) on the CPU; k / v are slices of a longer buffer."""
    gen = torch.Generator().manual_seed(seed)
    B, L = len(lens), kv_cap + 9                              # allocated positions; [kv_cap, L) are out of range
    lens = torch.tensor(lens)
    base = torch.tensor(win_base if isinstance(win_base, tuple) else (win_base,) * B)
    q = torch.randn(B, R, Hq, D, generator=gen).to(dtype).transpose(1, 2)
    kbuf, vbuf = (torch.randn(B, Hkv, L + 8, D, generator=gen).to(dtype) for _ in range(2))
    limit = (torch.rand(B, R, generator=gen) * (lens[:, None] + 1)).long().clamp(max=lens[:, None])
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, R), generator=gen, dtype=torch.int64)
    if R >= 5:
        limit[:, 0], bits[:, 1] = 0, -1                       # a row of window keys only; all 64 bits
        limit[:, 2] = torch.minimum(lens, base + 5)           # the union: the limit reaches into the window
        bits[:, 3] = 0
        limit[:, 4], bits[:, 4] = 0, 0                        # nothing visible: zeros
    else:
        limit[:, 0] = torch.maximum(limit[:, 0], lens.clamp(max=1))   # a visible key wherever there is one
    j = torch.arange(L)
    rel = (j - base[:, None, None]).clamp(0, 63)
    in_win = ((bits[:, :, None] >> rel) & 1).bool() & (j >= base[:, None, None]) & (j < base[:, None, None] + 64)
    visible = ((j < limit[:, :, None]) | in_win) & (j < lens[:, None, None])
    dead = ~visible.any(1)                                    # [B, L]: no row of the sequence sees the position
    for buf in (kbuf, vbuf):
        buf[:, :, 5:5 + L][dead[:, None, :].expand(B, Hkv, L)] = float("nan")
    return q, kbuf[:, :, 5:5 + L], vbuf[:, :, 5:5 + L], limit.int(), bits, visible


def _reference(q, k, v, visible, scale):
    """fp64: out[b, r, h] = sum_j softmax_j(scale q.k_j over the visible j) v_j, zeros where nothing is visible."""
    G = q.shape[1] // k.shape[1]
    kd, vd = (t.double().nan_to_num(0.0).repeat_interleave(G, 1) for t in (k, v))
    s = (q.double() @ kd.transpose(2, 3)) * scale
    p = s.masked_fill(~visible[:, None], float("-inf")).softmax(-1).nan_to_num(0.0)
    return (p @ vd).transpose(1, 2)


def _on_device(q, k, v, limit, bits):
    kd, vd = (torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV).copy_(t) for t in (k, v))
    return q.to(DEV), kd, vd, limit.to(DEV), bits.to(DEV)


def _long(values, add=0):
    return torch.tensor([x - add for x in values], dtype=torch.long, device=DEV)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x).replace("torch.", "").replace(" ", "") for x in c))
def test_ragged_lengths_match_the_fp64_reference(case):
    from specdec_amd import ops
    dtype, D, Hq, Hkv, R, lens, kv_cap, chunk_tiles, win_base, (len_add, base_add) = case
    B = len(lens)
    q, k, v, limit, bits, visible = _case(dtype, D, Hq, Hkv, R, lens, kv_cap, win_base)
    want = _reference(q, k, v, visible, D ** -0.5)
    kv_len = _long(lens, len_add)
    base = win_base
    if isinstance(win_base, tuple):                           # per sequence; else a host int, expanded on the device
        base = _long(win_base, base_add)
        base = kv_len if torch.equal(base, kv_len) else base  # one tensor for both, as a cache's cumulative_length
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.tree_attention(*_on_device(q, k, v, limit, bits), base, kv_len=kv_len, kv_cap=kv_cap, chunk_tiles=chunk_tiles,
                             kv_len_add=len_add, win_base_add=base_add, status_or=status)
    assert out.shape == (B, R, Hq, D) and out.dtype == dtype
    got = out.cpu().double()
    seen = visible.any(1)[:, None, :, None].expand(B, Hkv, k.shape[2], D)
    tol = 2 * torch.finfo(dtype).eps * float(v[seen].double().abs().max())
    err = float((got - want).abs().max())
    print(f"[tree-attn-ragged] {case}: chunks {ops.tree_attention_chunks(B, Hkv, kv_cap, chunk_tiles)}, max err {err:.3g}, tol {tol:.3g}")
    assert torch.isfinite(got).all()
    assert err <= tol
    assert int(status.item()) == 0
    assert not got[torch.tensor(lens) == 0].any()             # an empty sequence: zeros
    if R >= 5:
        assert not got[:, 4].any()                            # the row that sees nothing


@pytest.mark.parametrize("lens, kv_cap, chunk_tiles", [((1, 64, 333), 333, 1), ((40, 64), 64, 0)], ids=["chunks6", "chunks1"])
def test_a_sequence_does_not_depend_on_the_rest_of_the_batch(lens, kv_cap, chunk_tiles):
    from specdec_amd import ops
    q, k, v, limit, bits = _on_device(*_case(BF, 128, 4, 1, 29, lens, kv_cap, 30, seed=2)[:5])
    kw = dict(kv_cap=kv_cap, chunk_tiles=chunk_tiles)
    assert ops.tree_attention_chunks(len(lens), 1, kv_cap, chunk_tiles) == ops.tree_attention_chunks(1, 1, kv_cap, chunk_tiles)
    batch = ops.tree_attention(q, k, v, limit, bits, 30, kv_len=_long(lens), **kw)
    for b in range(len(lens)):
        s = slice(b, b + 1)
        alone = ops.tree_attention(q[s], k[s], v[s], limit[s].contiguous(), bits[s].contiguous(), 30, kv_len=_long(lens[s]), **kw)
        assert torch.equal(alone.view(torch.int16), batch[s].view(torch.int16)), b


def test_a_captured_call_follows_lengths_windows_and_rows_written_in_place():
    from specdec_amd import ops
    B, R, cap = 2, 29, 333
    steps = [((70, 10), (64, 5)), ((200, 129), (190, 100)), ((333, 300), (301, 250))]     # (lengths, window bases)
    q, k, v, _, _ = _on_device(*_case(BF, 128, 4, 1, R, (cap,) * B, cap, 0, seed=4)[:5])
    k, v = k.nan_to_num(0.5), v.nan_to_num(0.25)              # every position below kv_cap finite: the steps see different ones
    kv_len, base = _long(steps[0][0]), _long(steps[0][1])
    limit = torch.zeros(B, R, dtype=torch.int32, device=DEV)
    bits = torch.zeros(B, R, dtype=torch.long, device=DEV)
    out = torch.empty(B, R, 4, 128, dtype=BF, device=DEV)

    def call(o=None):
        return ops.tree_attention(q, k, v, limit, bits, base, kv_len=kv_len, kv_cap=cap, out=o)

    assert ops.tree_attention_chunks(B, 1, cap) > 1
    graph = None
    for i, (lens, bases) in enumerate(steps):
        _, _, _, lim_i, bits_i, _ = _case(BF, 128, 4, 1, R, lens, cap, bases, seed=10 + i)
        kv_len.copy_(_long(lens)), base.copy_(_long(bases)), limit.copy_(lim_i), bits.copy_(bits_i)
        eager = call()
        if graph is None:                                     # captured on the first step's values only
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call(out)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert eager.float().abs().sum() > 0
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), i


def test_statuses():
    from specdec_amd import _lib, ops
    q, k, v, limit, bits = _on_device(*_case(BF, 64, 4, 2, 8, (333, 100), 333, 90, seed=5)[:5])
    k, v = k.nan_to_num(0.5), v.nan_to_num(0.25)
    # a length above kv_cap: flagged, and clamped
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    over = ops.tree_attention(q, k, v, limit, bits, 90, kv_len=_long((500, 100)), kv_cap=333, chunk_tiles=2, status_or=status)
    clamped = ops.tree_attention(q, k, v, limit, bits, 90, kv_len=_long((333, 100)), kv_cap=333, chunk_tiles=2, status_or=None)
    assert int(status.item()) == BAD and torch.equal(over.view(torch.int16), clamped.view(torch.int16))
    # a pinned chunk length that needs 65 slots; a workspace one byte short
    long_k = torch.zeros(2, 2, 64 * 65, 64, dtype=BF, device=DEV)
    with pytest.raises(_lib.SpecdecError, match=r"\(-4\)"):
        ops.tree_attention(q, long_k, long_k, limit, bits, 0, kv_len=_long((5, 5)), chunk_tiles=1)
    need = _lib.lib.sd_tree_attention_ragged_workspace_size(2, 4, 2, 8, 64, 333, 2)
    with pytest.raises(_lib.SpecdecError, match=r"\(-2\)"):
        ops.tree_attention(q, k, v, limit, bits, 0, kv_len=_long((5, 5)), kv_cap=333, chunk_tiles=2,
                           workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))
    # a null kv_len_dev, through the C ABI: everything else valid
    a = _lib.sd_tree_attention_ragged_args()
    a.batch, a.heads_q, a.heads_kv, a.rows, a.head_dim, a.dtype, a.kv_cap, a.kv_alloc = 2, 4, 2, 8, 64, _lib.SD_BF16, 64, 342
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), over.data_ptr()
    a.q_stride_b, a.q_stride_h, a.q_stride_r = q.stride()[:3]
    a.k_stride_b, a.k_stride_h, a.k_stride_pos = a.v_stride_b, a.v_stride_h, a.v_stride_pos = k.stride()[:3]
    a.out_stride_b, a.out_stride_r, a.out_stride_h = over.stride()[:3]
    a.kv_limit, a.win_bits, a.win_base_dev, a.scale = limit.data_ptr(), bits.data_ptr(), bits.data_ptr(), 0.125
    assert _lib.lib.sd_tree_attention_ragged(C.byref(a), None) == _lib.SD_ERR_INVALID
