"""GPU tests of sd_tree_attention (ops.tree_attention, csrc/tree_attention.hip) against an fp64 torch
reference computed on the CPU from the same 16-bit inputs: the definition of include/specdec.h written
out plainly.  Every K/V position that no row of its sequence sees, and every position at or beyond
kv_len, holds NaN, so a kernel that reads one of them into the result fails the finiteness check.

Tolerance (derived): with eps = finfo(dtype).eps the unit roundoff is eps / 2; rounding P
to 16 bits moves an output by at most (eps / 2) max|V|, rounding the output by as much again, fp32
accumulation and exp2 are orders of magnitude below.  Bound eps max|V|; the tests allow 2 eps max|V|,
max|V| over the visible keys of the case."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16

# (dtype, D, Hq, Hkv, R, kv_len, splits, win_base, B, q transposed, reach: the largest kv_limit)
CASES = [
    (BF, 64, 2, 2, 1, 1, 0, 0, 1, False, None),
    (HF, 128, 4, 1, 29, 63, 0, 0, 1, False, None),
    (BF, 128, 8, 2, 33, 64, 0, 61, 1, True, None),            # the window cut off by kv_len
    (HF, 64, 8, 2, 65, 65, 0, 0, 3, False, None),
    (BF, 64, 4, 1, 128, 333, 1, 77, 1, False, None),          # 512 query rows: four passes of the row tiles
    (BF, 128, 8, 2, 128, 333, 2, 330, 1, True, None),
    (HF, 128, 2, 2, 29, 333, 5, 77, 3, False, None),          # spans of 1, 1, 1, 1 and 2 tiles, the last partial
    (BF, 64, 8, 2, 65, 333, 5, 77, 1, True, None),
    (BF, 128, 4, 1, 33, 333, 0, 0, 1, False, None),           # the split count by the shapes
    (HF, 64, 2, 2, 1, 333, 2, 330, 1, False, None),
    (BF, 128, 4, 1, 29, 333, 5, 77, 1, False, 100),           # spans beyond every row's reach
]


def _case(dtype, D, Hq, Hkv, R, kv_len, win_base, B, transposed, reach, seed=0):
    """(q, k, v, kv_limit, win_bits, visible [B, R, L] bool) on the CPU; k / v slices of a longer buffer."""
    gen = torch.Generator().manual_seed(seed)
    L = kv_len + 9                                            # allocated positions; [kv_len, L) are out of range
    q = torch.randn(B, R, Hq, D, generator=gen).to(dtype)
    q = q.transpose(1, 2) if transposed else q.transpose(1, 2).contiguous()
    kbuf, vbuf = (torch.randn(B, Hkv, L + 8, D, generator=gen).to(dtype) for _ in range(2))
    limit = torch.randint(0, (reach or kv_len) + 1, (B, R), generator=gen)
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, R), generator=gen, dtype=torch.int64)
    if R >= 5:
        limit[:, 0], bits[:, 1] = 0, -1                       # a row of window keys only; all 64 bits
        limit[:, 2] = min(kv_len, win_base + 5)               # the union: the limit reaches into the window
        bits[:, 3] = 0
        limit[:, 4], bits[:, 4] = 0, 0                        # nothing visible: zeros
    else:
        limit[:, 0].clamp_(min=1)                             # every sequence has a visible key
    j = torch.arange(L)
    rel = (j - win_base).clamp(0, 63)
    in_win = ((bits[:, :, None] >> rel) & 1).bool() & (j >= win_base) & (j < win_base + 64)
    visible = ((j < limit[:, :, None]) | in_win) & (j < kv_len)
    dead = ~visible.any(1)                                    # [B, L]: no row of the sequence sees the position
    for buf in (kbuf, vbuf):
        buf[:, :, 5:5 + L][dead[:, None, :].expand(B, Hkv, L)] = float("nan")
    return q, kbuf[:, :, 5:5 + L], vbuf[:, :, 5:5 + L], limit.int(), bits, visible


def _reference(q, k, v, visible, scale):
    """fp64: out[b, r, h] = sum_j softmax_j(scale q.k_j over the visible j) v_j, zeros where nothing is visible."""
    G = q.shape[1] // k.shape[1]
    kd, vd = (t.double().nan_to_num(0.0).repeat_interleave(G, 1) for t in (k, v))   # masked entries never count
    s = (q.double() @ kd.transpose(2, 3)) * scale
    p = s.masked_fill(~visible[:, None], float("-inf")).softmax(-1).nan_to_num(0.0)
    return (p @ vd).transpose(1, 2)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x).replace("torch.", "") for x in c))
def test_tree_attention_matches_the_fp64_reference(case):
    from specdec_amd import ops
    dtype, D, Hq, Hkv, R, kv_len, splits, win_base, B, transposed, reach = case
    q, k, v, limit, bits, visible = _case(dtype, D, Hq, Hkv, R, kv_len, win_base, B, transposed, reach)
    want = _reference(q, k, v, visible, D ** -0.5)
    qd = q.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) if transposed else q.to(DEV)
    kd, vd = (torch.empty_strided(t.shape, t.stride(), dtype=dtype, device=DEV).copy_(t) for t in (k, v))
    out = ops.tree_attention(qd, kd, vd, limit.to(DEV), bits.to(DEV), win_base, kv_len=kv_len, splits=splits)
    assert out.shape == (B, R, Hq, D) and out.dtype == dtype
    got = out.cpu().double()
    seen = visible.any(1)[:, None, :, None].expand(B, Hkv, k.shape[2], D)
    vmax = float(v[seen].double().abs().max())
    tol = 2 * torch.finfo(dtype).eps * vmax
    err = float((got - want).abs().max())
    print(f"[tree-attn] {case}: splits {ops.tree_attention_splits(B, Hkv, kv_len, splits)}, max err {err:.3g}, tol {tol:.3g}")
    assert torch.isfinite(got).all()
    assert err <= tol
    if R >= 5:
        assert not got[:, 4].any()                            # the row that sees nothing


@pytest.mark.parametrize("change, status", [
    (dict(dtype=torch.float32), -4), (dict(D=96), -4), (dict(R=129), -4), (dict(Hq=3, Hkv=2), -1),
    (dict(short_workspace=True), -2)])
def test_argument_errors_return_statuses(change, status):
    """fp32, D = 96 and R = 129: SD_ERR_UNSUPPORTED; Hq no multiple of Hkv: SD_ERR_INVALID; a workspace one
    byte short: SD_ERR_WORKSPACE.  The wrapper raises the library's status."""
    from specdec_amd import _lib, ops
    c = dict(dtype=BF, D=64, Hq=4, Hkv=2, R=8, short_workspace=False)
    c.update(change)
    q = torch.zeros(1, c["Hq"], c["R"], c["D"], dtype=c["dtype"], device=DEV)
    k = torch.zeros(1, c["Hkv"], 333, c["D"], dtype=c["dtype"], device=DEV)
    limit = torch.zeros(1, c["R"], dtype=torch.int32, device=DEV)
    ws = None
    if c["short_workspace"]:
        need = _lib.lib.sd_tree_attention_workspace_size(1, c["Hq"], c["Hkv"], c["R"], c["D"], 333, 2)
        ws = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.SpecdecError, match=rf"\({status}\)"):
        ops.tree_attention(q, k, k, limit, limit.long(), 0, splits=2, workspace=ws)


@pytest.mark.parametrize("splits", [0, 2])
def test_a_captured_call_replays_the_eager_result_bit_for_bit(splits):
    from specdec_amd import ops
    q, k, v, limit, bits, _ = _case(BF, 128, 4, 1, 29, 333, 77, 1, False, None, seed=3)
    q, k, v, limit, bits = (t.to(DEV) for t in (q, k.contiguous(), v.contiguous(), limit, bits))
    eager = ops.tree_attention(q, k, v, limit, bits, 77, kv_len=333, splits=splits)
    out = torch.empty_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.tree_attention(q, k, v, limit, bits, 77, kv_len=333, splits=splits, out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
