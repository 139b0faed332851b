"""GPU tests of the paged-cache entries (sd_tree_attention_paged, sd_kv_store_paged, sd_kv_compact_paged; ops.tree_attention
and ops.kv_compact with ``block_table``, ops.kv_store_paged).  A contiguous ragged case of tests/test_gpu_tree_attention_ragged.py
is scattered into a pool through a random permutation of page ids: the pool has more pages than are used, every unused page
and every slot at or beyond len_b (and every position no row sees) holds NaN (FP8: the NaN byte), and block-table entries
at or beyond ceil(len_b / S) are -1.  Reference: fp64 attention over the visible keys.

Tolerance (unchanged): 2 eps max|V| over the visible keys; FP8: V = v_scale * e4m3 value."""
import functools

import pytest
import torch

import kv_ref
from test_gpu_tree_attention_ragged import BAD, BF, DEV, HF, _case, _long, _reference

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    t.view(torch.uint8).fill_(0x7f) if dtype == F8 else t.fill_(float("nan"))
    return t


def _pool(seq, lens, S, place, num_pages, psh=False):
    """Scatter seq [B, H, L, D] (CPU) into a NaN pool [num_pages, H, S, D]: page p of sequence b goes to place[b][p]."""
    B, H, L, D = seq.shape
    pool = _poison((num_pages, S, H, D), seq.dtype).permute(0, 2, 1, 3) if psh else _poison((num_pages, H, S, D), seq.dtype)
    padded = torch.cat([_bytes(seq), _bytes(_poison((B, H, len(place[0]) * S - L, D), seq.dtype))], 2)   # bytes: any dtype
    table = torch.full((B, len(place[0])), -1, dtype=torch.int32)
    for b in range(B):
        for p in range(-(-lens[b] // S)):
            _bytes(pool)[place[b][p]] = padded[b, :, p * S:(p + 1) * S]
            table[b, p] = place[b][p]
    return pool, table


def _places(B, max_pages, seed):
    """(identity, permuted, pool pages): page p of sequence b at b * max_pages + p, or at a random page of a larger pool."""
    num_pages = B * max_pages + 3
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed))[:B * max_pages].view(B, max_pages).tolist()
    return torch.arange(B * max_pages).view(B, max_pages).tolist(), perm, num_pages


def _dev(t):
    return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV).copy_(t)


def _bytes(t):
    return t.view(torch.uint8 if t.element_size() == 1 else torch.int16)


def _quantised(k, v, Hkv):
    """(k8, v8, k_scale, v_scale, dequantised k, v) of a 16-bit case; a NaN position becomes the NaN byte."""
    ks, vs = torch.linspace(0.02, 0.05, Hkv), torch.linspace(0.04, 0.01, Hkv)
    k8, v8 = ((t.float() / s[None, :, None, None]).clamp(-448, 448).to(F8) for t, s in ((k, ks), (v, vs)))
    return k8, v8, ks, vs, k8.float().double() * ks[None, :, None, None].double(), v8.float().double() * vs[None, :, None, None].double()


# (dtype, FP8 pools, D, Hq, Hkv, R, lengths, S, chunk_tiles, window bases, [P, S, Hkv, D] pool)
CASES = [
    (BF, False, 64, 2, 2, 1, (0, 1, 65, 333), 16, 1, (0, 0, 60, 300), False),     # a tile over four pages; an empty sequence
    (HF, False, 128, 4, 1, 29, (0, 1, 65, 333), 64, 2, (0, 0, 3, 330), False),    # a tile is a page
    (BF, False, 128, 8, 2, 65, (0, 1, 65, 333), 128, 0, (0, 0, 50, 290), True),   # two tiles in a page; the permuted pool
    (HF, False, 64, 4, 2, 65, (64, 128, 129), 16, 2, (60, 100, 120), True),       # ends on a page border and one past it
    (BF, False, 64, 2, 1, 29, (64, 128, 129), 128, 1, (0, 100, 128), False),      # a chunk starts mid-page (S = 128, 1 tile)
    (BF, False, 128, 4, 1, 1, (64, 128, 129), 64, 0, 0, False),
    (BF, True, 64, 4, 2, 29, (0, 1, 65, 333), 16, 1, (0, 0, 60, 300), False),
    (HF, True, 128, 4, 1, 65, (0, 1, 65, 333), 64, 0, (0, 0, 3, 330), True),
    (BF, True, 128, 8, 2, 1, (64, 128, 129), 128, 2, (60, 100, 120), False),
    (HF, True, 64, 2, 2, 65, (64, 128, 129), 16, 2, 100, True),
    (HF, False, 128, 2, 2, 29, (0, 1, 65, 333), 16, 0, (0, 0, 60, 300), False),
    (BF, True, 64, 2, 1, 29, (64, 128, 129), 128, 1, (0, 100, 128), False),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x).replace("torch.", "").replace(" ", "") for x in c))
def test_paged_attention_matches_the_fp64_reference_in_any_placement(case):
    from specdec_amd import ops
    dtype, fp8, D, Hq, Hkv, R, lens, S, chunk_tiles, win_base, psh = case
    B, cap = len(lens), max(lens)
    q, k, v, limit, bits, visible = _case(dtype, D, Hq, Hkv, R, lens, cap, win_base)
    scales, kr, vr = {}, k, v
    if fp8:
        k, v, ks, vs, kr, vr = _quantised(k, v, Hkv)
        scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    want = _reference(q, kr, vr, visible, D ** -0.5)
    ident, perm, num_pages = _places(B, -(-k.shape[2] // S), seed=R)
    base = _long(win_base) if isinstance(win_base, tuple) else win_base
    outs = []
    for place in (perm, ident):
        (kp, table), (vp, _) = (_pool(t, lens, S, place, num_pages, psh) for t in (k, v))
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        outs.append(ops.tree_attention(q.to(DEV), _dev(kp), _dev(vp), limit.to(DEV), bits.to(DEV), base, kv_len=_long(lens),
                                       kv_cap=cap, chunk_tiles=chunk_tiles, status_or=status, block_table=table.to(DEV), **scales))
        assert int(status.item()) == 0
    got = outs[0].cpu().double()
    seen = visible.any(1)[:, None, :, None].expand(B, Hkv, k.shape[2], D)
    tol = 2 * torch.finfo(dtype).eps * float(vr[seen].double().abs().max())
    err = float((got - want).abs().max())
    print(f"[tree-attn-paged] {case}: chunks {ops.tree_attention_chunks(B, Hkv, cap, chunk_tiles)}, max err {err:.3g}, tol {tol:.3g}")
    assert outs[0].shape == (B, R, Hq, D) and torch.isfinite(got).all()
    assert err <= tol
    assert not got[torch.tensor(lens) == 0].any()             # an empty sequence: zeros
    assert torch.equal(_bytes(outs[0]), _bytes(outs[1]))      # the same arithmetic at other addresses


def test_a_captured_paged_call_follows_lengths_windows_and_table_rows_written_in_place():
    from specdec_amd import ops
    B, R, cap, S = 2, 29, 333, 16
    steps = [((70, 10), (64, 5)), ((200, 129), (190, 100)), ((333, 300), (301, 250))]     # (lengths, window bases)
    q, k, v, _, _, _ = _case(BF, 128, 4, 1, R, (cap,) * B, cap, 0, seed=4)
    k, v = k.nan_to_num(0.5), v.nan_to_num(0.25)
    _, perm, num_pages = _places(B, -(-k.shape[2] // S), seed=7)
    (kp, t0), (vp, _) = (_pool(t, (cap,) * B, S, perm, num_pages) for t in (k, v))
    t1 = t0.flip(0).contiguous()                              # the sequences trade their pages
    q, kp, vp = q.to(DEV), _dev(kp), _dev(vp)
    kv_len, base, table = _long(steps[0][0]), _long(steps[0][1]), t0.to(DEV)
    limit = torch.zeros(B, R, dtype=torch.int32, device=DEV)
    bits = torch.zeros(B, R, dtype=torch.long, device=DEV)
    out = torch.empty(B, R, 4, 128, dtype=BF, device=DEV)

    def call(o=None):
        return ops.tree_attention(q, kp, vp, limit, bits, base, kv_len=kv_len, kv_cap=cap, out=o, block_table=table)

    graph = None
    for i, (lens, bases) in enumerate(steps):
        _, _, _, lim_i, bits_i, _ = _case(BF, 128, 4, 1, R, lens, cap, bases, seed=10 + i)
        kv_len.copy_(_long(lens)), base.copy_(_long(bases)), limit.copy_(lim_i), bits.copy_(bits_i), table.copy_((t0, t1)[i % 2])
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


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("bad_id", [-1, "num_pages"])
def test_a_page_id_out_of_range_is_refused(fp8, bad_id):
    from specdec_amd import ops
    lens, S, R = (100, 333, 65), 16, 8
    q, k, v, limit, bits, _ = _case(BF, 64, 4, 2, R, lens, 333, 90, seed=5)
    scales = {}
    if fp8:
        k, v, ks, vs, _, _ = _quantised(k, v, 2)
        scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    _, perm, num_pages = _places(3, -(-k.shape[2] // S), seed=1)
    (kp, table), (vp, _) = (_pool(t, lens, S, perm, num_pages) for t in (k, v))
    kp, vp = _dev(kp), _dev(vp)
    kp0, vp0 = kp.clone(), vp.clone()
    args = (q.to(DEV), kp, vp, limit.to(DEV), bits.to(DEV), 90)
    kw = dict(kv_len=_long(lens), kv_cap=333, chunk_tiles=2, **scales)
    clean = ops.tree_attention(*args, block_table=table.to(DEV), **kw)
    table[1, 3] = num_pages if bad_id == "num_pages" else bad_id     # keys 48..63 of sequence 1: inside its length
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.tree_attention(*args, block_table=table.to(DEV), status_or=status, **kw)
    assert int(status.item()) == BAD
    assert torch.isfinite(out[1].float()).all()
    assert torch.equal(_bytes(out[[0, 2]]), _bytes(clean[[0, 2]]))
    assert torch.equal(_bytes(kp), _bytes(kp0)) and torch.equal(_bytes(vp), _bytes(vp0))


def _gather(pool, table, S):
    """The logical cache [B, H, max_pages * S, D] a table describes (entries -1 read page 0: never compared)."""
    pages = _bytes(pool)[table.clamp(min=0).long()]           # [B, max_pages, H, S, D], as bytes: any dtype
    return pages.permute(0, 2, 1, 3, 4).reshape(table.shape[0], pool.shape[1], -1, pool.shape[3]).view(pool.dtype)


# A chunk of more than 1024 pages: a workgroup stages the first 1024 ids of its chunk and reads the ids behind them
# from the table as it goes.  The smallest such chunk: S = 16 and 260 tiles, 1040 pages.
LONG_TILES, LONG_S = 260, 16
LONG_KEYS = LONG_TILES * 64


@functools.lru_cache(maxsize=None)
def _long_case(fp8, chunks):
    """One case per (pool type, chunk count), built and referenced once: sequence 0 ends five keys into page 1024 of
    its last chunk, sequence 1 at kv_cap (its window lies on the pages 1029..1033 of that chunk), sequence 2 stays
    below 1024 pages."""
    c0, cap = (chunks - 1) * LONG_KEYS, chunks * LONG_KEYS
    lens, bases = (c0 + 1024 * LONG_S + 5, cap, 1000), (c0 + 1024 * LONG_S - 4, c0 + 1029 * LONG_S + 6, 900)
    dtype = HF if fp8 else BF
    q, k, v, limit, bits, visible = _case(dtype, 64, 2, 1, 3, lens, cap, bases, seed=9)
    assert visible[0, :, c0 + 1024 * LONG_S:].any() and visible[1, :, c0 + 1030 * LONG_S:c0 + 1031 * LONG_S].any()
    scales, kr, vr = {}, k, v
    if fp8:
        k, v, ks, vs, kr, vr = _quantised(k, v, 1)
        scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    want = _reference(q, kr, vr, visible, 64 ** -0.5)
    seen = visible.any(1)[:, None, :, None].expand(3, 1, k.shape[2], 64)
    tol = 2 * torch.finfo(dtype).eps * float(vr[seen].double().abs().max())
    _, perm, num_pages = _places(3, -(-k.shape[2] // LONG_S), seed=chunks)
    (kp, table), (vp, _) = (_pool(t, lens, LONG_S, perm, num_pages) for t in (k, v))
    args = (q.to(DEV), _dev(kp), _dev(vp), limit.to(DEV), bits.to(DEV), _long(bases))
    kw = dict(kv_len=_long(lens), kv_cap=cap, chunk_tiles=LONG_TILES, **scales)
    return args, kw, table, num_pages, want, tol


@pytest.mark.parametrize("chunks", [1, 2], ids=["direct", "chunks2"])
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_page_ids_behind_the_staged_ones_are_read_from_the_table(fp8, chunks):
    from specdec_amd import ops
    args, kw, table, _, want, tol = _long_case(fp8, chunks)
    assert ops.tree_attention_chunks(3, 1, kw["kv_cap"], LONG_TILES) == chunks
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.tree_attention(*args, block_table=table.to(DEV), status_or=status, **kw)
    assert int(status.item()) == 0
    got = out.cpu().double()
    err = float((got - want).abs().max())
    print(f"[tree-attn-paged] long chunk fp8={fp8} chunks={chunks}: max err {err:.3g}, tol {tol:.3g}")
    assert torch.isfinite(got).all() and err <= tol
    # the contiguous ragged call on the cache the table describes: the same arithmetic
    q, kp, vp, limit, bits, base = args
    flat = ops.tree_attention(q, _gather(kp, table.to(DEV), LONG_S), _gather(vp, table.to(DEV), LONG_S), limit, bits, base, **kw)
    assert torch.equal(_bytes(out), _bytes(flat))


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_a_page_id_out_of_range_behind_the_staged_ones_is_refused(fp8):
    from specdec_amd import ops
    args, kw, table, num_pages, _, _ = _long_case(fp8, 1)
    clean = ops.tree_attention(*args, block_table=table.to(DEV), **kw)
    bad = table.clone()
    bad[1, 1030] = num_pages                                  # keys 16480..16495 of sequence 1: inside its window
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.tree_attention(*args, block_table=bad.to(DEV), status_or=status, **kw)
    assert int(status.item()) == BAD
    assert torch.isfinite(out[1].float()).all()
    assert torch.equal(_bytes(out[[0, 2]]), _bytes(clean[[0, 2]]))


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_store_writes_the_rows_and_nothing_else(fp8):
    from specdec_amd import ops
    B, H, R, D, S, max_pages = 2, 2, 29, 64, 16, 5
    gen = torch.Generator().manual_seed(3)
    k_new, v_new = (torch.randn(B, R, H, D, generator=gen).to(BF).transpose(1, 2).to(DEV) for _ in range(2))
    _, perm, num_pages = _places(B, max_pages, seed=2)
    table = torch.tensor(perm, dtype=torch.int32)
    pos = torch.tensor([5, 40])                               # rows 5..33 and 40..68: four and three page borders crossed
    dtype = F8 if fp8 else BF
    pools = [_poison((num_pages, H, S, D), dtype).to(DEV) for _ in range(2)]
    want = [p.cpu() for p in pools]
    scales, rows = {}, (k_new.cpu(), v_new.cpu())
    if fp8:
        scales = dict(k_scale=torch.tensor([0.03, 0.011], device=DEV), v_scale=torch.tensor([0.02, 0.04], device=DEV))
        flat = [torch.zeros(B, H, R, D, dtype=F8, device=DEV) for _ in range(2)]
        ops.kv_store_fp8(k_new, v_new, flat[0], flat[1], scales["k_scale"], scales["v_scale"], 0)
        rows = [t.cpu() for t in flat]
    for w, x in zip(want, rows):
        for b in range(B):
            for r in range(R):
                p = int(pos[b]) + r
                _bytes(w)[perm[b][p // S], :, p % S] = _bytes(x)[b, :, r]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_store_paged(k_new, v_new, pools[0], pools[1], table.to(DEV), pos.to(DEV), status_or=status, **scales)
    assert int(status.item()) == 0
    for got, w in zip(pools, want):
        assert torch.equal(_bytes(got.cpu()), _bytes(w))
    # rows beyond the table, and a refused page id (rows 64..68 of sequence 1): skipped and reported; the rows that
    # are written rewrite their own bytes, so the pools stay what they were
    bad_table = table.clone()
    bad_table[0, 0] = num_pages
    for pos_bad, tab in ((torch.tensor([5, 80]), table), (pos, bad_table)):
        ops.kv_store_paged(k_new, v_new, pools[0], pools[1], tab.to(DEV), pos_bad.to(DEV), status_or=status, **scales)
        assert int(status.item()) == BAD
        status.zero_()
        for got, w in zip(pools, want):
            assert torch.equal(_bytes(got.cpu()), _bytes(w))


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_store_attend_compact_attend(fp8):
    from specdec_amd import ops
    B, Hq, H, R, D, S, max_pages = 2, 4, 2, 29, 64, 16, 5
    lens, dtype = (21, 40), F8 if fp8 else BF                 # window bases mid-page: the tree spans three pages
    gen = torch.Generator().manual_seed(6)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(BF)
    ks, vs = (torch.tensor(x) for x in (([0.03, 0.011], [0.02, 0.04]) if fp8 else ([1.0, 1.0], [1.0, 1.0])))
    scales = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV)) if fp8 else {}
    _, perm, num_pages = _places(B, max_pages, seed=8)
    table = torch.tensor(perm, dtype=torch.int32).to(DEV)
    pools = []
    for s in (ks, vs):                                        # the prefixes, placed by the host
        pre = rnd(B, H, max_pages * S, D)
        pre = (pre.float() / s[None, :, None, None]).to(F8) if fp8 else pre
        for b in range(B):
            _bytes(pre)[b, :, lens[b]:] = _bytes(_poison((1,), dtype))[0]
        pools.append(_pool(pre, lens, S, perm, num_pages)[0].to(DEV))
    k_new, v_new = (rnd(B, R, H, D).transpose(1, 2).to(DEV) for _ in range(2))
    ops.kv_store_paged(k_new, v_new, pools[0], pools[1], table, _long(lens), **scales)

    def check(tag, q, kv_len, limit, bits, base):
        out = ops.tree_attention(q.to(DEV), pools[0], pools[1], limit.int().to(DEV), bits.to(DEV), _long(base),
                                 kv_len=_long(kv_len), block_table=table, **scales).cpu().double()
        L = max_pages * S
        kd, vd = (_gather(p.cpu(), table.cpu(), S).float().double() * s[None, :, None, None].double() for p, s in zip(pools, (ks, vs)))
        j = torch.arange(L)
        rel = (j - torch.tensor(base)[:, None, None]).clamp(0, 63)
        visible = ((j < limit[:, :, None]) | (((bits[:, :, None] >> rel) & 1).bool() & (j >= torch.tensor(base)[:, None, None])))
        visible &= j < torch.tensor(kv_len)[:, None, None]
        want = _reference(q, kd, vd, visible, D ** -0.5)
        tol = 2 * torch.finfo(BF).eps * float(vd[visible.any(1)[:, None, :, None].expand_as(vd)].abs().max())
        err = float((out - want).abs().max())
        print(f"[tree-attn-paged] {tag} fp8={fp8}: max err {err:.3g}, tol {tol:.3g}")
        assert torch.isfinite(out).all() and err <= tol

    # the tree forward: node r (parent (r - 1) // 2) sees the prefix, its ancestors and itself
    anc = [0] * R
    for r in range(R):
        anc[r] = (1 << r) | (anc[(r - 1) // 2] if r else 0)
    bits = torch.tensor([anc] * B, dtype=torch.int64)
    limit = torch.tensor(lens)[:, None].expand(B, R)
    check("tree", rnd(B, R, Hq, D).transpose(1, 2), [n + R for n in lens], limit, bits, list(lens))
    # the accepted path 0 -> 2 -> 6 -> 14: slot 14 (page of base + 14) moves to depth 3, across a page border
    path = torch.tensor([[0, 2, 6, 14], [0, 1, 4, -1]], dtype=torch.int32)
    count = torch.tensor([4, 3], dtype=torch.int32)
    want = [_bytes(_gather(p.cpu(), table.cpu(), S)) for p in pools]
    for b in range(B):
        kv_ref.compact([w[b:b + 1] for w in want], path[b:b + 1], count[b:b + 1], lens[b], R)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_compact(pools, path.to(DEV), count.to(DEV), 0, num_slots=R, base_dev=_long(lens), status_or=status, block_table=table)
    assert int(status.item()) == 0
    for p, w in zip(pools, want):
        assert torch.equal(_bytes(_gather(p.cpu(), table.cpu(), S)), w)
    # catch-up rows over the committed tokens: row i sees the prefix and the first i + 1 accepted tokens
    new_len = [n + int(c) for n, c in zip(lens, count)]
    limit = torch.minimum(torch.tensor(lens)[:, None] + torch.arange(1, 5), torch.tensor(new_len)[:, None])
    check("catch-up", rnd(B, 4, Hq, D).transpose(1, 2), new_len, limit, torch.zeros(B, 4, dtype=torch.int64), new_len)
