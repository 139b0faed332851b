"""GPU tests of sd_kv_compact (csrc/kv_compact.hip) through ops.kv_compact and utils.caching.compact_cache.

Every case is compared BIT FOR BIT with the host model (tests/kv_ref.py) run on a copy: the tensors are
strided views into one buffer of random 16-bit words (the poison), each between guard bands, and the
WHOLE buffer must equal the host model's afterwards — so every byte outside the destination rows is
checked too: positions >= base + count, the padding between heads and sequences, the guard bands."""
import copy

import pytest
import torch

import kv_ref
import tree_walk as tw

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                   # 16-bit words before and after every tensor
BAD = 0x40                                   # SD_ROW_INVALID_DIST


def _plan(n, B, H, L, D, dtype, layout, off2=False):
    """(total 16-bit words, [(word offset, shape, element strides)]) of n tensors [B, H, L, D] in one
    buffer.  layout: "packed"; "static" (the L positions are the front of a 96-position buffer);
    "padb" (13 spare elements after every sequence).  off2: every tensor starts 2 bytes off a 16-byte
    boundary."""
    w = torch.empty(0, dtype=dtype).element_size() // 2          # 16-bit words per element
    Lbuf = 96 if layout == "static" else L
    sh, sb = Lbuf * D, H * Lbuf * D + (13 if layout == "padb" else 0)
    words = B * sb * w
    at, views = 0, []
    for _ in range(n):
        at += GUARD
        at = (at + 7) // 8 * 8 + (1 if off2 else 0)               # 16-byte aligned (+ 2 bytes)
        views.append((at, (B, H, L, D), (sb, sh, D, 1)))
        at += words
    return at + GUARD, views


def _views(buf, plan, dtype):
    w = torch.empty(0, dtype=dtype).element_size() // 2
    total, views = plan
    out = []
    for at, shape, strides in views:
        n_el = (shape[0] - 1) * strides[0] + (shape[1] - 1) * strides[1] + (shape[2] - 1) * strides[2] + shape[3]
        out.append(buf[at:at + n_el * w].view(dtype).as_strided(shape, strides))
    return out


def _run(plan, dtype, path, count, base, num_slots, node_slot=None, use_base_dev=False, seed=0):
    """One kv_compact call on a fresh poisoned buffer against the host model on its copy; returns the
    status word.  path: [B][depth] lists."""
    from specdec_amd import ops
    g = torch.Generator().manual_seed(seed)
    host = torch.randint(-32768, 32767, (plan[0],), generator=g, dtype=torch.int16)
    dev = host.to(DEV)
    p_host, c_host = torch.tensor(path, dtype=torch.int32), torch.tensor(count, dtype=torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(base_dev=torch.tensor([base], dtype=torch.long, device=DEV)) if use_base_dev else {}
    ops.kv_compact(_views(dev, plan, dtype), p_host.to(DEV), c_host.to(DEV), 0 if use_base_dev else base,
                   num_slots=num_slots, node_slot=node_slot, status_or=status, **kw)
    flagged = kv_ref.compact(_views(host, plan, dtype), p_host, c_host, base, num_slots, node_slot)
    got = dev.cpu()
    diff = (got != host).nonzero().flatten()
    assert diff.numel() == 0, f"{diff.numel()} words differ from the host model, first at {int(diff[0])}"
    st = int(status.item())
    assert st == (BAD if flagged else 0), (st, flagged)
    return st


N10 = tw.from_branching([2, 2, 1])           # 10 nodes: 0 1 | 2 3 4 5 | 6 7 8 9
SHIFT = list(range(1, 32))                   # chains(1, 32) fed with an offset of one: everything moves down by one


def _scenarios():
    """(name, path [B][depth], count [B], base, num_slots, node_slot, base_dev?)"""
    perm = [3, 0, 7, 1, 9, 2, 8, 4, 6, 5]    # node -> slot, a permutation with slot(path[d]) >= d on the paths below
    return [
        ("count0", [[0, 2, 6]], [0], 7, 10, None, False),
        ("identity", [[0, 1, 2]], [3], 7, 10, None, False),
        ("path", [[0, 3, 7]], [3], 7, 10, None, False),
        ("last-node", [[1, 5, 9]], [3], 30, 10, None, False),             # the window ends with the cache
        ("minus-one-past-n", [[1, 4, -1]], [2], 0, 10, None, False),
        ("shift", [SHIFT], [31], 7, 32, None, False),                     # the hazard: dst(d) = src(d - 1)
        ("shift-short", [SHIFT], [9], 8, 32, None, False),                # one full group of depths and one more
        ("batch3", [[0, 2, 6], [1, 5, -1], [1, 4, 8]], [0, 2, 3], 11, 10, None, False),
        ("node-slot", [[0, 2, 6], [1, 4, 8], [0, 3, 7]], [3, 3, 2], 5, 10, perm, False),
        ("base-dev", [[1, 4, 8], [0, 3, -1], [1, -1, -1]], [3, 2, 1], 19, 10, None, True),
        ("corrupt-node-64", [[1, 64, 8]], [3], 7, 10, None, False),       # ends the moves at depth 1, status set
        ("corrupt-slot", [[0, 9, 6], [1, 4, 8]], [3, 3], 7, 9, None, False),   # slot 9 >= num_slots 9
        ("corrupt-slot-map", [[0, 3, 7]], [3], 7, 10, [5, 0, 0, 0, 0, 0, 0, 64], False),   # slot 0 < depth 1
        ("count-past-n", [[0, 3, -1]], [3], 7, 10, None, False),          # count says depth 2 moves, the path does not
        ("count-past-depth", [[0, 3, 7]], [40], 7, 10, None, False),      # min(count, depth): no error
        ("negative-count", [[0, 3, 7]], [-2], 7, 10, None, False),
    ]


SHAPES = {"h2-d128-bf16": (2, 128, torch.bfloat16, False), "h2-d8-fp32": (2, 8, torch.float32, False),
          "h3-d5-bf16": (3, 5, torch.bfloat16, False),          # 10-byte rows: the 2-byte path, a row ending inside its chunk
          "h1-d64-fp16": (1, 64, torch.float16, False),
          "h2-d24-bf16-off2": (2, 24, torch.bfloat16, True),    # every address 2 bytes off: the 2-byte path on 48-byte rows
          "h2-d12-bf16": (2, 12, torch.bfloat16, False),        # 24-byte rows: the 8-byte path, 16 + 8 bytes
          "h2-d3-fp32": (2, 3, torch.float32, False)}           # 12-byte rows: the 4-byte path


@pytest.mark.parametrize("layout", ["packed", "static", "padb"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_scenario_equals_the_host_model_bit_for_bit(shape, layout):
    H, D, dtype, off2 = SHAPES[shape]
    statuses = {}
    for i, (name, path, count, base, slots, node_slot, bdev) in enumerate(_scenarios()):
        plan = _plan(2, len(count), H, 40, D, dtype, layout, off2)
        statuses[name] = _run(plan, dtype, path, count, base, slots, node_slot, bdev, seed=i)
    assert {k for k, v in statuses.items() if v} == {"corrupt-node-64", "corrupt-slot", "corrupt-slot-map", "count-past-n"}


@pytest.mark.parametrize("n", [64, 300])
def test_many_tensors_in_one_call_and_a_list_the_wrapper_splits(n):
    plan = _plan(n, 1, 2, 40, 16, torch.bfloat16, "packed")
    assert _run(plan, torch.bfloat16, [[1, 5, 9]], [3], 7, 10) == 0
    assert _run(plan, torch.bfloat16, [SHIFT], [31], 3, 32, seed=1) == 0


def test_a_64_node_tree_and_its_deepest_paths():
    from specdec_amd.tree import TokenTree
    tree = TokenTree(tw.TREES["irregular64"])
    plan = _plan(2, 3, 2, 80, 8, torch.bfloat16, "padb")
    leaves = sorted(range(64), key=lambda i: -tree.node_depth[i])[:2] + [63]
    paths = [tree.path_to(i) for i in leaves]
    pad = [p + [-1] * (tree.depth - len(p)) for p in paths]
    assert _run(plan, torch.bfloat16, pad, [len(p) for p in paths], 16, 64) == 0


def test_a_window_that_leaves_the_cache_moves_nothing():
    """base comes from the device here, so only the kernel can see that [base, base + num_slots) leaves
    the 40 positions: nothing moves and the status word says so.  The wrapper refuses a host base."""
    from specdec_amd import ops
    plan = _plan(2, 1, 2, 40, 8, torch.bfloat16, "packed")
    host = torch.randint(-32768, 32767, (plan[0],), dtype=torch.int16, generator=torch.Generator().manual_seed(5))
    for base in (31, -1):
        dev = host.to(DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.kv_compact(_views(dev, plan, torch.bfloat16), torch.tensor([[1, 5, 9]], dtype=torch.int32, device=DEV),
                       torch.tensor([3], dtype=torch.int32, device=DEV), 0, num_slots=10, status_or=status,
                       base_dev=torch.tensor([base], dtype=torch.long, device=DEV))
        assert torch.equal(dev.cpu(), host) and int(status.item()) == BAD, base
    with pytest.raises(ValueError):
        ops.kv_compact(_views(host.to(DEV), plan, torch.bfloat16), torch.zeros(1, 3, dtype=torch.int32, device=DEV),
                       torch.zeros(1, dtype=torch.int32, device=DEV), 31, num_slots=10)


def test_a_captured_call_replays_with_new_path_count_and_base():
    """Captured once over a static-style buffer with base_dev; each replay sees other device contents of
    path, count and base_dev and must equal the host model on them."""
    from specdec_amd import ops
    dtype = torch.bfloat16
    plan = _plan(4, 2, 2, 40, 64, dtype, "static")
    init = torch.randint(-32768, 32767, (plan[0],), dtype=torch.int16, generator=torch.Generator().manual_seed(9))
    buf = init.to(DEV)
    views = _views(buf, plan, dtype)
    path = torch.full((2, 3), -1, dtype=torch.int32, device=DEV)
    count = torch.zeros(2, dtype=torch.int32, device=DEV)
    bdev = torch.zeros(1, dtype=torch.long, device=DEV)
    ops.kv_compact(views, path, count, 0, num_slots=10, base_dev=bdev)          # eager once (count 0: nothing moves)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.kv_compact(views, path, count, 0, num_slots=10, base_dev=bdev)
    for p, c, base in (([[1, 4, 8], [0, 2, -1]], [3, 2], 5), ([[1, 5, 9], [1, 4, 8]], [1, 3], 30)):
        buf.copy_(init)
        path.copy_(torch.tensor(p, dtype=torch.int32))
        count.copy_(torch.tensor(c, dtype=torch.int32))
        bdev.fill_(base)
        graph.replay()
        torch.cuda.synchronize()
        want = init.clone()
        assert not kv_ref.compact(_views(want, plan, dtype), p, c, base, 10)
        assert torch.equal(buf.cpu(), want) and not torch.equal(want, init), (p, c, base)


def test_verify_tree_then_kv_compact_without_a_host_read():
    """Greedy rows (fp32, V = 64) built so that sequence 0 accepts nothing, sequence 1 one node and sequence 2 a whole
    path; verify_tree's path and n_accepted go straight into kv_compact, and the host model is fed the
    same outputs afterwards."""
    from specdec_amd import ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    tree, B, V = TokenTree(N10), 3, 64
    g = torch.Generator().manual_seed(4)
    target = torch.randn(B, tree.num_nodes + 1, V, generator=g)
    # a slot's children are draws from its drafter row: the target's row where the children are to be
    # accepted, that row rolled by one (another argmax) where they are to be rejected
    draft = torch.empty(B, len(tree.internal_slots), V)
    tokens = torch.zeros(B, tree.num_nodes, dtype=torch.long)
    for b, right_depths in enumerate((0, 1, 3)):
        for k, s in enumerate(tree.internal_slots):
            child_depth = 1 if s == 0 else tree.node_depth[s - 1] + 1
            draft[b, k] = target[b, s] if child_depth <= right_depths else target[b, s].roll(1)
            tokens[b, tree.children[s]] = draft[b, k].argmax()
    dtype = torch.bfloat16
    plan = _plan(6, B, 2, 40, 16, dtype, "packed")
    init = torch.randint(-32768, 32767, (plan[0],), dtype=torch.int16, generator=g)
    buf = init.to(DEV)
    out = ops.verify_tree(target.to(DEV), draft.to(DEV), tokens.to(DEV), tree, ops.ProcSpec("greedy", 1.0), PhiloxNoise(seed=3))
    ops.kv_compact(_views(buf, plan, dtype), out.path, out.n_accepted, 12, num_slots=tree.num_nodes)
    torch.cuda.synchronize()
    n, path = out.n_accepted.cpu(), out.path.cpu()
    assert n.tolist() == [0, 1, 3] and path[2].tolist() == [0, 2, 6] and path[1, 0] == 0
    want = init.clone()
    assert not kv_ref.compact(_views(want, plan, dtype), path, n, 12, tree.num_nodes)
    assert torch.equal(buf.cpu(), want)


# ---------------------------------------------------------------- utils.caching.compact_cache
def _kv(seed, L=20):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 2, L, 8, generator=g).to(DEV), torch.randn(2, 2, L, 8, generator=g).to(DEV)) for _ in range(3)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(kv_ref.cache_tensors(a), kv_ref.cache_tensors(b)))


@pytest.mark.parametrize("node_slot", [None, [0, 2, 1, 3, 4]], ids=["identity", "fed-by-level"])
def test_compact_cache_dispatches_on_the_cache_type_and_sets_the_length(node_slot):
    transformers = pytest.importorskip("transformers")
    from transformers.cache_utils import DynamicCache, StaticCache
    from specdec_amd.utils.caching import compact_cache
    path = torch.tensor([[2, 3], [0, 4]], dtype=torch.int32, device=DEV)        # nodes of the tree [-1, 0, -1, 2, 0]
    count = torch.tensor([2, 2], dtype=torch.int32, device=DEV)
    base, slots, new = 15, 5, 17
    # a tuple cache: compacted in place, sliced views returned
    tup = tuple(_kv(1))
    ref = kv_ref.compact_cache(tuple(tuple(t.clone() for t in layer) for layer in tup), path, count, base, slots, node_slot, new)
    got = compact_cache(tup, path, count, base, num_slots=slots, node_slot=node_slot, new_length=new)
    assert _same(got, ref) and got[0][0].shape[2] == new and not torch.equal(tup[0][0][:, :, base], _kv(1)[0][0][:, :, base])
    # a DynamicCache: compacted, then cropped with the negative form
    dyn = DynamicCache()
    for i, (k, v) in enumerate(_kv(2)):
        dyn.update(k, v, i)
    ref = kv_ref.compact_cache(copy.deepcopy(dyn), path, count, base, slots, node_slot, new)
    assert compact_cache(dyn, path, count, base, num_slots=slots, node_slot=node_slot, new_length=new) is dyn
    assert _same(dyn, ref) and dyn.get_seq_length() == new and dyn.layers[2].keys.shape[2] == new
    # a StaticCache: compacted, cumulative_length set on the device from count (no host value given) or from new_length
    cfg = transformers.LlamaConfig(vocab_size=32, hidden_size=16, intermediate_size=32, num_hidden_layers=3,
                                   num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=64)
    for given in (None, new):
        st = StaticCache(config=cfg, max_cache_len=32)
        for i, (k, v) in enumerate(_kv(3)):
            st.update(k, v, i)
        ref = kv_ref.compact_cache(copy.deepcopy(st), path, count, base, slots, node_slot, new)
        ptrs = [t.data_ptr() for t in kv_ref.cache_tensors(st)]
        assert compact_cache(st, path, count, base, num_slots=slots, node_slot=node_slot, new_length=given) is st
        assert _same(st, ref) and [t.data_ptr() for t in kv_ref.cache_tensors(st)] == ptrs
        assert [int(layer.cumulative_length) for layer in st.layers] == [new] * 3
        assert st.layers[0].cumulative_length.dtype == torch.int64
    with pytest.raises(ValueError, match="Unsupported cache type."):
        compact_cache(object(), path, count, base, num_slots=slots, new_length=new)
