"""CPU checks of the KV-cache compaction: the ctypes mirror against the header, the torch op's
registration and fake trace, the host model (tests/kv_ref.py) against the torch expression of the move
and on the in-place hazard, the wrappers' refusals (they are GPU-only like the rest of the package: the
move itself is tested in tests/test_gpu_kv_compact.py), and the host model on a 2-layer fp64 Llama —
compact and continue equals the uncached forward, for DynamicCache and StaticCache."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

import kv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- struct layout, constants, exports
def test_kv_compact_args_ctypes_layout_matches_the_header():
    from specdec_amd import _lib
    s = "sd_kv_compact_args"
    old = ["sd_verify_args", "sd_sample_args", "sd_ngram_args", "sd_beam_args", "sd_multi_args", "sd_vp_args", "sd_tree_args"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "specdec.h"\nint main(void) {\n'
    prog += f'  printf("{s}.size %zu\\n", sizeof({s}));\n'
    for f, _ in _lib.sd_kv_compact_args._fields_:
        prog += f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n'
    for o in old:
        prog += f'  printf("{o}.size %zu\\n", sizeof({o}));\n'
    prog += ('  printf("limits %d %d %d\\n", SD_KV_MAX_TENSORS, SD_TREE_MAX_NODES, SD_MAX_GAMMA);\n'
             '  printf("abi %d\\n", SD_ABI_VERSION);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = dict(line.split(" ", 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got[f"{s}.size"]) == C.sizeof(_lib.sd_kv_compact_args)
    for f, _ in _lib.sd_kv_compact_args._fields_:
        assert getattr(_lib.sd_kv_compact_args, f).offset == int(got[f"{s}.{f}"]), f
    assert got["limits"].split() == ["256", "64", "32"] and _lib.SD_KV_MAX_TENSORS == 256
    assert got["abi"] == "12" and _lib.SD_ABI_VERSION == 12 and _lib.lib.sd_abi_version() == 12
    for o in old:                                        # additive: the existing structs keep their sizes
        assert int(got[f"{o}.size"]) == C.sizeof(getattr(_lib, o)), o
    assert "sd_kv_compact" in _lib.EXPORTS and hasattr(_lib.lib, "sd_kv_compact")


def test_argument_checks_refuse_before_any_launch():
    """Every call here is refused on the host (the pointers are fakes); tests/asan/kv_asan.cpp drives the
    full list under AddressSanitizer."""
    from specdec_amd import _lib
    lib = _lib.lib

    def call(n_tensors=4, **kw):
        a = _lib.sd_kv_compact_args()
        table = (C.c_void_p * max(n_tensors, 1))(*[0x100000 + 0x1000 * t for t in range(max(n_tensors, 1))])
        a.n_tensors, a.batch, a.heads, a.max_depth, a.num_slots, a.row_bytes = n_tensors, 1, 2, 3, 10, 16
        a.tensors = table
        a.stride_pos, a.stride_h, a.stride_b = 16, 40 * 16, 2 * 40 * 16
        a.num_positions, a.base = 40, 7
        a.path, a.path_stride_b, a.count = 0x200000, 3, 0x201000
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sd_kv_compact(C.byref(a), None)

    INV, UNS = _lib.SD_ERR_INVALID, _lib.SD_ERR_UNSUPPORTED
    assert lib.sd_kv_compact(None, None) == INV
    assert call(n_tensors=0) == INV and call(n_tensors=257) == UNS and call(tensors=None) == INV
    assert call(row_bytes=0) == INV and call(row_bytes=15) == INV and call(row_bytes=-16) == INV
    assert call(stride_b=-8) == INV and call(stride_h=-8) == INV and call(stride_pos=-16) == INV and call(stride_pos=8) == INV
    assert call(max_depth=0) == INV and call(max_depth=33, path_stride_b=33) == UNS
    assert call(num_slots=0) == INV and call(num_slots=65, num_positions=100) == UNS
    assert call(base=-1) == INV and call(base=31) == INV and call(num_positions=9, base=0) == INV
    assert call(path=None) == INV and call(count=None) == INV and call(path_stride_b=2) == INV
    assert call(batch=2 ** 31 - 1, heads=2 ** 16) == UNS          # a grid beyond the launch limit


# ---------------------------------------------------------------- the torch op
def test_kv_compact_op_registers_and_traces_with_fake_tensors():
    import specdec_amd  # noqa: F401
    schema = str(torch.ops.specdec.kv_compact.default._schema)
    assert schema.startswith("specdec::kv_compact(Tensor(a0!)[] tensors, Tensor path, Tensor count,") and schema.endswith("-> ()")
    with torch._subclasses.FakeTensorMode():
        tensors = [torch.empty(1, 2, 40, 8, dtype=torch.bfloat16) for _ in range(4)]
        path, count = torch.empty(1, 3, dtype=torch.int32), torch.empty(1, dtype=torch.int32)
        assert torch.ops.specdec.kv_compact(tensors, path, count, 7, 10) is None
        assert torch.ops.specdec.kv_compact(tensors, path, count, 0, 10, node_slot=[1, 0, 2],
                                            base_dev=torch.empty(1, dtype=torch.long)) is None


# ---------------------------------------------------------------- the host model
def _cache(B=1, H=2, L=40, D=4, n=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, L, D, generator=g, dtype=torch.float64) for _ in range(n)]


def test_host_model_equals_the_torch_expression_on_increasing_paths():
    """index_select then index_copy_ (gather everything, then scatter) is the sequential loop's result on a
    strictly increasing path — whatever the overlaps, since every source lies at or above its depth."""
    for path in ([0, 1, 2], [1, 2, 3], [0, 2, 5], [3, 7, 9], [9], [1, 2, 3, 4, 5, 6, 7, 8, 9]):
        ts = _cache()
        want = [t.clone() for t in ts]
        idx = torch.tensor(path)
        for t in want:
            t.index_copy_(2, 7 + torch.arange(len(path)), t.index_select(2, 7 + idx))
        pad = torch.full((1, 10), -1, dtype=torch.int32)
        pad[0, :len(path)] = idx.int()
        assert not kv_ref.compact(ts, pad, [len(path)], 7, 10)
        for a, b in zip(ts, want):
            assert torch.equal(a, b), path


def test_host_model_walks_depths_in_order_and_stops_at_bad_entries():
    ts = _cache(B=3)
    ref = [t.clone() for t in ts]
    path = torch.tensor([[5, 6, 7, -1], [2, 1, 3, -1], [4, 64, 1, -1]], dtype=torch.int32)
    flagged = kv_ref.compact(ts, path, [0, 3, 3], 10, 8)
    assert flagged
    for t, r in zip(ts, ref):
        assert torch.equal(t[0], r[0])                                       # count 0: untouched
        assert torch.equal(t[1, :, 10], r[1, :, 12]) and torch.equal(t[1, :, 11], r[1, :, 11])   # slot 1 at depth 1: in place
        assert torch.equal(t[1, :, 12], r[1, :, 13])
        assert torch.equal(t[2, :, 10], r[2, :, 14]) and torch.equal(t[2, :, 11:], r[2, :, 11:])   # 64 ends the row
        assert torch.equal(t[:, :, :10], r[:, :, :10]) and torch.equal(t[:, :, 18:], r[:, :, 18:])
    # a slot below its depth and a slot at num_slots end the moves; a count past the path is no error
    for path, count, flag in (([[1, 0, 2]], [3], True), ([[1, 8]], [2], True), ([[1, 2]], [5], False)):
        ts = _cache()
        ref = [t.clone() for t in ts]
        assert kv_ref.compact(ts, torch.tensor(path, dtype=torch.int32), count, 3, 8) == flag
        assert torch.equal(ts[0][0, :, 3], ref[0][0, :, 4])                  # depth 0 moved in all three
        if flag:                                                             # depth 1 ended the moves
            assert torch.equal(ts[0][0, :, 4:], ref[0][0, :, 4:])
        else:                                                                # min(count, depth) = 2: no error
            assert torch.equal(ts[0][0, :, 4], ref[0][0, :, 5]) and torch.equal(ts[0][0, :, 5:], ref[0][0, :, 5:])


def test_host_model_node_slot_maps_nodes_to_cache_order():
    """The tree [-1, 0, -1, 2, 0] fed level by level enters the cache in the order 0, 2, 1, 3, 4."""
    slot = [0, 2, 1, 3, 4]
    ts = _cache()
    ref = [t.clone() for t in ts]
    assert not kv_ref.compact(ts, torch.tensor([[2, 3]], dtype=torch.int32), [2], 5, 5, node_slot=slot)
    for t, r in zip(ts, ref):
        assert torch.equal(t[0, :, 5], r[0, :, 6]) and torch.equal(t[0, :, 6], r[0, :, 8])
    assert kv_ref.compact(_cache(), torch.tensor([[0, 1]], dtype=torch.int32), [2], 5, 5, node_slot=[1, 0])   # slot 0 at depth 1
    assert kv_ref.compact(_cache(), torch.tensor([[3]], dtype=torch.int32), [1], 5, 5, node_slot=[0, 1])      # no slot for node 3


# ---------------------------------------------------------------- the wrappers refuse what they cannot serve
def test_wrappers_refuse_bad_tensors_and_unknown_caches():
    from specdec_amd import ops
    from specdec_amd.utils.caching import compact_cache
    path, count = torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    good = _cache(n=2)
    for bad in ([], [good[0], good[1][:, :1]], [good[0], good[1].float()], [good[0].transpose(2, 3)],
                [good[0][..., ::2]], [good[0][0]], [torch.zeros(1, 2, 40, 3, dtype=torch.int8)], good):   # the last: host tensors
        with pytest.raises(ValueError):
            ops.kv_compact(bad, path, count, 7, num_slots=10)
    for cache in (object(), [good], {"k": good}, None):
        with pytest.raises(ValueError, match="Unsupported cache type."):
            compact_cache(cache, path, count, 7, num_slots=10, new_length=9)
    with pytest.raises(ValueError, match="new_length"):
        compact_cache((tuple(good),), path, count, 7, num_slots=10)


# ---------------------------------------------------------------- the host model on a real model
def _llama():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=97, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64)
    cfg._attn_implementation = "eager"
    torch.manual_seed(0)
    return transformers.LlamaForCausalLM(cfg).double().eval()


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("parent,feed", [([-1, -1, 0, 0, 1, 2, 2, 4], None), ([-1, 0, -1, 2, 0], [0, 2, 1, 3, 4])],
                         ids=["level-ordered", "fed-by-level"])
def test_compact_and_continue_equals_the_uncached_forward(kind, parent, feed):
    """A cache holding the committed tokens but the root takes a tree-masked forward over root + nodes
    (fed in index order, or level by level so that the node -> slot map is no identity): its logits equal
    the uncached tree forward's.  After the host model compacts every path onto the front and sets the
    length, a plain cached forward of the next token equals the uncached forward over prefix + path + token.
    Both within 1e-7 (fp64 rounding of a 2-layer model is below 1e-12; a wrong slot moves logits by 1e-2)."""
    from transformers.cache_utils import DynamicCache, StaticCache
    from specdec_amd.sampling.tree_decoding import _allowed
    from specdec_amd.tree import TokenTree
    model, tree = _llama(), TokenTree(parent)
    N, width = tree.num_nodes, 32
    order = list(range(N)) if feed is None else feed
    slot = [order.index(i) for i in range(N)]
    prefix = torch.tensor([[5, 17, 33, 2, 60]])
    P = prefix.shape[1]
    nodes = torch.tensor([[11 + i for i in range(N)]])
    fmin = torch.finfo(torch.float64).min
    with torch.no_grad():
        full_mask, full_pos = tree.attention_inputs(P, torch.float64)
        uncached = model(input_ids=torch.cat([prefix, nodes], 1), attention_mask=full_mask, position_ids=full_pos).logits[0]

    def tree_cache():
        cache = DynamicCache(config=model.config) if kind == "dynamic" else StaticCache(config=model.config, max_cache_len=width)
        kw = lambda a, b: dict(cache_position=torch.arange(a, b)) if kind == "static" else {}   # noqa: E731
        allow, pos = _allowed(tree, P, P - 1, order, slot)
        mask = torch.full((1 + N, width if kind == "static" else P + N), fmin, dtype=torch.float64)
        mask[:, :P + N].masked_fill_(allow, 0)
        with torch.no_grad():
            model(input_ids=prefix[:, :P - 1], past_key_values=cache, use_cache=True, **kw(0, P - 1))
            out = model(input_ids=torch.cat([prefix[:, P - 1:], nodes[:, order]], 1), attention_mask=mask[None, None],
                        position_ids=pos, past_key_values=cache, use_cache=True, **kw(P - 1, P + N))
        return cache, out.logits[0], kw

    _, logits, _ = tree_cache()
    rows = [P - 1] + [P + i for i in order]
    assert float((logits - uncached[rows]).abs().max()) < 1e-7
    if feed is None:                                                    # the loop's rows are attention_inputs' rows
        allow, pos = _allowed(tree, P, P - 1, order, slot)
        assert torch.equal(allow, full_mask[0, 0, P - 1:] == 0) and torch.equal(pos, full_pos[:, P - 1:])
    worst = 0.0
    for leaf in range(N):
        path = tree.path_to(leaf)
        for n in range(len(path) + 1):
            cache, _, kw = tree_cache()
            pt = torch.full((1, tree.depth), -1, dtype=torch.int32)
            pt[0, :n] = torch.tensor(path[:n], dtype=torch.int32)
            cache = kv_ref.compact_cache(cache, pt, [n], P, N, None if feed is None else slot, new_length=P + n)
            assert int(cache.get_seq_length()) == P + n
            nxt = torch.tensor([[70 + n]])
            with torch.no_grad():
                got = model(input_ids=nxt, past_key_values=cache, use_cache=True, **kw(P + n, P + n + 1)).logits[0, -1]
                want = model(input_ids=torch.cat([prefix, nodes[:, path[:n]], nxt], 1)).logits[0, -1]
            worst = max(worst, float((got - want).abs().max()))
    print(f"[kv-compact] {kind}: compact-and-continue differs from the uncached forward by {worst:.3g}")
    assert worst < 1e-7
