"""GPU tests of the quantising K/V store (sd_kv_store_fp8 through ops.kv_store_fp8, csrc/kv_store_fp8.hip): the
bytes it writes equal those of the CPU expression ``(x.float() / scale).clamp(-448, 448).to(float8_e4m3fn)``, no
byte outside the written rows changes, a row that leaves the cache is skipped and reported, and a stored cache
read back by tree_attention meets the fp64 reference of the quantised values."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
SENTINEL = 0x5A


def _scales(H):
    h = torch.arange(H, dtype=torch.float32)
    return 0.5 + 0.37 * h, 1.25 - 0.11 * h


def _rows(dtype, B, H, R, D, scale, seed):
    """New rows [B, H, R, D]: random values, and in the first elements of every row the edge cases: zeros, values
    beyond +-448 scale, +-inf, NaN, and the e4m3 subnormal steps and their ties (scale * k * 2^-10)."""
    x = (torch.randn(B, H, R, D, generator=torch.Generator().manual_seed(seed)) * 3).to(dtype)
    s = scale[None, :, None]
    x[..., 0], x[..., 1] = 0.0, -0.0
    x[..., 2], x[..., 3] = (500.0 * s).to(dtype), (-3000.0 * s).to(dtype)
    x[..., 4], x[..., 5], x[..., 6] = float("inf"), float("-inf"), float("nan")
    for k in range(1, 7):
        x[..., 6 + k] = (s * k * 2.0 ** -10 * (-1) ** k).to(dtype)
    return x


def _expect(x, scale):
    return (x.float() / scale[None, :, None, None]).clamp(-448, 448).to(F8).view(torch.uint8)


@pytest.mark.parametrize("pos_mode", ["host", "dev1", "devB"])
@pytest.mark.parametrize("B, R", [(1, 1), (3, 29)])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dtype, D", [(BF, 64), (HF, 128), (BF, 128), (HF, 64)])
def test_store_writes_the_bytes_of_the_cpu_expression_and_nothing_else(dtype, D, transposed, B, R, pos_mode):
    from specdec_amd import ops
    H, L = 2, 47
    ks, vs = _scales(H)
    kn, vn = _rows(dtype, B, H, R, D, ks, 1), _rows(dtype, B, H, R, D, vs, 2)
    starts = {"host": [7] * B, "dev1": [7 + 4] * B, "devB": [7 + 5 * b for b in range(B)]}[pos_mode]
    pos_dev = {"host": None, "dev1": torch.tensor([4]), "devB": torch.tensor([5 * b for b in range(B)])}[pos_mode]
    want = [torch.full((B, H, L, D), SENTINEL, dtype=torch.uint8) for _ in range(2)]
    for w, x, s in zip(want, (kn, vn), (ks, vs)):
        for b in range(B):
            w[b, :, starts[b]:starts[b] + R] = _expect(x[b:b + 1], s)[0]
    put = (lambda t: t.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)) if transposed else (lambda t: t.to(DEV))
    kc, vc = (torch.full((B, H, L, D), SENTINEL, dtype=torch.uint8, device=DEV).view(F8) for _ in range(2))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_store_fp8(put(kn), put(vn), kc, vc, ks.to(DEV), vs.to(DEV), 7,
                     pos_dev=None if pos_dev is None else pos_dev.to(DEV), status_or=status)
    assert torch.equal(kc.view(torch.uint8).cpu(), want[0])
    assert torch.equal(vc.view(torch.uint8).cpu(), want[1])
    assert int(status) == 0


def test_a_row_landing_at_L_is_not_written_and_sets_the_status_bit():
    from specdec_amd import _lib, ops
    B, H, R, D, L = 2, 2, 5, 64, 20
    ks, vs = _scales(H)
    kn, vn = _rows(BF, B, H, R, D, ks, 3), _rows(BF, B, H, R, D, vs, 4)
    kc, vc = (torch.full((B, H, L, D), SENTINEL, dtype=torch.uint8, device=DEV).view(F8) for _ in range(2))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    starts = [3, L - R + 1]                                   # the second sequence's last row would land at L
    ops.kv_store_fp8(kn.to(DEV), vn.to(DEV), kc, vc, ks.to(DEV), vs.to(DEV), 0, pos_dev=torch.tensor(starts, device=DEV),
                     status_or=status)
    want = torch.full((B, H, L, D), SENTINEL, dtype=torch.uint8)
    want[0, :, 3:3 + R] = _expect(kn[0:1], ks)[0]
    want[1, :, starts[1]:] = _expect(kn[1:2], ks)[0][:, :R - 1]
    assert torch.equal(kc.view(torch.uint8).cpu(), want)
    assert int(status) == _lib.SD_ROW_INVALID_DIST


def test_tree_attention_reads_what_the_store_wrote():
    """Store, then attend over the stored cache: against the fp64 reference of the quantised values, 2 eps max|V|."""
    from specdec_amd import ops
    B, Hq, H, R, D, L = 1, 4, 2, 29, 128, 96
    gen = torch.Generator().manual_seed(5)
    ks, vs = _scales(H)
    kn, vn = (torch.randn(B, H, L, D, generator=gen).to(BF) for _ in range(2))
    q = torch.randn(B, Hq, R, D, generator=gen).to(BF)
    kc, vc = (torch.zeros(B, H, L, D, dtype=torch.uint8, device=DEV).view(F8) for _ in range(2))
    ops.kv_store_fp8(kn.to(DEV), vn.to(DEV), kc, vc, ks.to(DEV), vs.to(DEV), 0)
    limit = torch.arange(L - R + 1, L + 1, dtype=torch.int32)[None]          # causal rows at the end of the cache
    out = ops.tree_attention(q.to(DEV), kc, vc, limit.to(DEV), torch.zeros(B, R, dtype=torch.int64, device=DEV), 0,
                             k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    kq, vq = ((x.float() / s[None, :, None, None]).clamp(-448, 448).to(F8).double() * s.double()[None, :, None, None]
              for x, s in ((kn, ks), (vn, vs)))
    G = Hq // H
    sc = (q.double() @ kq.repeat_interleave(G, 1).transpose(2, 3)) * D ** -0.5
    visible = torch.arange(L)[None, None] < limit[:, :, None]
    want = (sc.masked_fill(~visible[:, None], float("-inf")).softmax(-1) @ vq.repeat_interleave(G, 1)).transpose(1, 2)
    err, tol = float((out.cpu().double() - want).abs().max()), 2 * torch.finfo(BF).eps * float(vq.abs().max())
    print(f"[kv-store-fp8] round trip: max err {err:.3g}, tol {tol:.3g}")
    assert err <= tol
