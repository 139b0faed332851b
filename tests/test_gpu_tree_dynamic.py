"""GPU tests of the per-sequence tree verify (sd_verify_tree_dynamic; csrc/sd_verify_tree_dynamic.inc):
with one topology for every sequence it equals sd_verify_tree_distinct bit for bit on the cases of
tests/tree_distinct_walk.py (which test_gpu_tree_distinct.py holds to the host model); with a different
topology per sequence every row equals the B = 1 sd_verify_tree_distinct call of its own tree; invalid
device topologies flag exactly their rows; graph capture; the torch op."""
from types import SimpleNamespace

import pytest
import torch

import multi_walk as mw
import tree_distinct_walk as dw
import tree_walk as tw
from tree_ref import children_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = -7
FIELDS = ("n_accepted", "last_node", "next_token", "resample_mass", "n_sibling_rejects", "stop_index", "row_status",
          "path", "tokens_out")
B4 = 4


@pytest.fixture(scope="module")
def sd():
    from specdec_amd import _lib, ops
    from specdec_amd.noise import PhiloxNoise
    from specdec_amd.tree import TokenTree
    return SimpleNamespace(lib=_lib, ops=ops, PhiloxNoise=PhiloxNoise, TokenTree=TokenTree)


def spec_of(sd, p):
    return sd.ops.ProcSpec(p.kind, p.temperature, p.top_k, p.top_p)


def distinct(sd, tl, tok, parent, proc, off, row_base, stops=()):
    stop_t = torch.tensor(list(stops), dtype=torch.long, device=DEV)
    out = sd.ops.verify_tree_distinct(tl, tok, sd.TokenTree(parent), spec_of(sd, proc), sd.PhiloxNoise(seed=dw.SEED, offset=off),
                                      stop_tokens=stop_t, pad_token_id=PAD, row_base=row_base)
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})


def dynamic(sd, tl, tok, parent_dev, proc, off, row_base, max_depth, stops=(), status_or=None):
    stop_t = torch.tensor(list(stops), dtype=torch.long, device=DEV)
    out = sd.ops.verify_tree_dynamic(tl, tok, parent_dev, spec_of(sd, proc), sd.PhiloxNoise(seed=dw.SEED, offset=off), max_depth,
                                     stop_tokens=stop_t, status_or=status_or, pad_token_id=PAD, row_base=row_base)
    assert sd.lib.last_verify_path() == sd.lib.SD_PATH_VERIFY_TREE_DYNAMIC == 10
    return SimpleNamespace(**{f: getattr(out, f).cpu() for f in FIELDS})


def same(a, b):
    """Bit equality, NaN equal to NaN."""
    if a.dtype.is_floating_point:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def parents_dev(rows, width=None):
    """int32 [B, N] on the device; width: inside a wider buffer whose tail holds an invalid parent."""
    t = torch.tensor(rows, dtype=torch.int32)
    if width is None:
        return t.to(DEV)
    buf = torch.full((t.shape[0], width), 1 << 20, dtype=torch.int32)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]]


# ---------------------------------------------------------------- one topology: sd_verify_tree_distinct
SHAPES = {"multinomial": (2049, torch.bfloat16), "greedy": (4101, torch.float16), "nucleus0.9": (1000, torch.float32)}


@pytest.mark.parametrize("proc_name", list(SHAPES))
@pytest.mark.parametrize("tname", list(dw.TREES))
def test_one_topology_equals_verify_tree_distinct_bit_for_bit(sd, tname, proc_name):
    V, dtype = SHAPES[proc_name]
    c = dw.case(tname, V, dtype, proc_name)
    off, rows = dw.quiet_offset(c)                          # as the distinct suite chooses it
    stops = [int(c.tok[1, 0])] if tname != "one" else []
    tl, tok = c.tl[:B4].to(DEV), c.tok[:B4].contiguous().to(DEV)
    depth = max(tw.node_depths(c.parent))
    want = distinct(sd, tl, tok, c.parent, c.proc, off, dw.ROW_BASE, stops)
    got = dynamic(sd, tl, tok, parents_dev([c.parent] * B4), c.proc, off, dw.ROW_BASE, depth, stops)
    for f in FIELDS:
        assert same(getattr(got, f), getattr(want, f)), (f, getattr(got, f), getattr(want, f))
    assert bool((got.row_status & sd.lib.SD_ROW_DONE).all())


# ---------------------------------------------------------------- a topology per sequence
def embed(live, V, gen, N=64):
    """(parent [N], tok [N]): the `live` tree followed by nodes the walk can never accept — one child with
    an id outside the vocabulary (under the root, or under the last live node where the root is full)
    and an 8-ary subtree below it."""
    parent = list(live)
    tok = torch.randint(0, V, (N,), generator=gen)
    n0 = len(parent)
    if n0 < N:
        root_full = sum(p == -1 for p in parent) >= 8
        parent.append(n0 - 1 if root_full else -1)
        tok[n0] = V + 1
        for k in range(1, N - n0):
            parent.append(n0 + (k - 1) // 8)
    return parent, tok


LIVE = {"one": [-1], "chain32": tw.chains(1, 32), "irregular64": tw.irregular(), "fan8": tw.from_branching([8]),
        "five": [-1, -1, 0, 0, 1]}


@pytest.mark.parametrize("proc_name", list(SHAPES))
def test_a_topology_per_sequence_equals_the_single_calls(sd, proc_name):
    """B = 5, N = 64: a single live node, a chain of 32, the irregular 64-node tree, 8 children at the
    root and a 5-node tree (the rest of each: nodes that cannot be accepted), parent_dev with a row
    stride of 70.  Every row equals the B = 1 sd_verify_tree_distinct call of its own tree at row_base +
    b, every field, path and tokens_out filled with -1 / pad beyond the tree's own depth."""
    V, dtype = SHAPES[proc_name]
    proc = mw.PROCS[proc_name]
    gen = torch.Generator().manual_seed(77)
    trees = [embed(LIVE[k], V, gen) for k in LIVE]
    B, N, D = len(trees), 64, 32
    tok = torch.stack([t for _, t in trees])
    tl = torch.randn(B, N + 1, V, generator=gen) * 3
    for b, (parent, _) in enumerate(trees):                 # the first child of a slot: nearly all the row's mass, or a lift
        for s, cs in enumerate(children_of(parent)):
            if cs and 0 <= int(tok[b, cs[0]]) < V:
                if (s + b) % 3:
                    tl[b, s, int(tok[b, cs[0]])] = 20.0
                else:
                    tl[b, s, int(tok[b, cs[0]])] += 4.0
    tl, tok = tl.to(dtype).to(DEV), tok.to(DEV)
    off = dw.OFFSET
    got = dynamic(sd, tl, tok, parents_dev([p for p, _ in trees], width=70), proc, off, dw.ROW_BASE, D)
    depths = set()
    for b, (parent, _) in enumerate(trees):
        want = distinct(sd, tl[b:b + 1], tok[b:b + 1], parent, proc, off, dw.ROW_BASE + b)
        d = max(tw.node_depths(parent))
        for f in FIELDS[:7]:
            assert same(getattr(got, f)[b:b + 1], getattr(want, f)), (b, f, getattr(got, f)[b], getattr(want, f))
        assert got.path[b, :d].tolist() == want.path[0].tolist() and got.path[b, d:].tolist() == [-1] * (D - d), b
        assert got.tokens_out[b, :d + 1].tolist() == want.tokens_out[0].tolist(), b
        assert got.tokens_out[b, d + 1:].tolist() == [PAD] * (D - d), b
        depths.add(int(got.n_accepted[b]))
    print(f"[tree-dynamic] {proc_name}: accepted depths {got.n_accepted.tolist()}")
    assert int(got.n_accepted[0]) <= 1                      # one live node


# ---------------------------------------------------------------- invalid device topologies
def test_invalid_topologies_flag_exactly_their_rows(sd):
    L = sd.lib
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    depth = max(tw.node_depths(c.parent))
    dep = tw.node_depths(c.parent)
    deepest = [i for i, d in enumerate(dep) if d == depth]
    assert len(deepest) >= 2
    bad = {1: list(c.parent), 3: list(c.parent), 5: [-1] * 9 + list(c.parent[9:]), 7: list(c.parent)}
    bad[1][5] = 5                                           # its own parent
    bad[3][3] = -2                                          # below -1
    bad[7][deepest[1]] = deepest[0]                         # one node deeper than max_depth
    assert max(len(k) for k in children_of(bad[5])) >= 9 and max(tw.node_depths(bad[7])) == depth + 1
    rows = [bad.get(b, c.parent) for b in range(c.B)]
    tl, tok = c.tl.to(DEV), c.tok.to(DEV)
    tok0 = tok.clone()
    off, _ = dw.quiet_offset(c)
    want = dynamic(sd, tl, tok, parents_dev([c.parent] * c.B), c.proc, off, dw.ROW_BASE, depth)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pd = parents_dev(rows, width=67)
    whole = pd._base.clone() if pd._base is not None else None
    got = dynamic(sd, tl, tok, pd, c.proc, off, dw.ROW_BASE, depth, status_or=err)
    for b in range(c.B):
        if b in bad:
            assert int(got.row_status[b]) == L.SD_ROW_DONE | L.SD_ROW_INVALID_DIST, (b, hex(int(got.row_status[b])))
            assert int(got.n_accepted[b]) == 0 and int(got.next_token[b]) == -1 and int(got.last_node[b]) == -1
            assert got.path[b].tolist() == [-1] * depth and got.tokens_out[b].tolist() == [PAD] * (depth + 1)
            assert int(got.stop_index[b]) == -1 and int(got.n_sibling_rejects[b]) == 0
            assert bool(got.resample_mass[b].isnan())
        else:                                               # unchanged, every field
            for f in FIELDS:
                assert same(getattr(got, f)[b], getattr(want, f)[b]), (b, f)
            assert not int(got.row_status[b]) & L.SD_ROW_ERROR_MASK
    assert int(err[0]) == L.SD_ROW_INVALID_DIST
    assert torch.equal(tok, tok0) and (whole is None or torch.equal(pd._base, whole))
    # a valid call leaves the sticky word alone
    err.zero_()
    dynamic(sd, tl, tok, parents_dev([c.parent] * c.B), c.proc, off, dw.ROW_BASE, depth, status_or=err)
    assert int(err[0]) == 0
    # depth exactly max_depth and 8 children are taken
    got = dynamic(sd, tl[:1, :9], tok[:1, :8].contiguous(), parents_dev([[-1] * 8]), c.proc, off, 0, 1)
    assert not int(got.row_status[0]) & L.SD_ROW_ERROR_MASK


# ---------------------------------------------------------------- call-level checks
def test_capture_and_replay_with_an_advanced_offset(sd):
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    tl, tok = c.tl.to(DEV), c.tok.to(DEV)
    depth = max(tw.node_depths(c.parent))
    alt = [(i - 1) // 2 for i in range(64)]                 # a second topology: the binary tree, depth 6
    rows = [alt if b % 2 else c.parent for b in range(c.B)]
    assert depth <= 8
    pd = parents_dev(rows)
    D = 8
    spec = spec_of(sd, c.proc)
    off = torch.tensor([0], dtype=torch.long, device=DEV)
    noise = sd.PhiloxNoise(seed=dw.SEED, offset=0, offset_dev=off)   # the eager call takes host offset 0, the captured one 1
    eager = sd.ops.verify_tree_dynamic(tl, tok, pd, spec, noise, D, pad_token_id=PAD, row_base=dw.ROW_BASE)   # sizes the workspace
    want0 = {f: getattr(eager, f).clone() for f in FIELDS}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sd.ops.verify_tree_dynamic(tl, tok, pd, spec, noise, D, pad_token_id=PAD, row_base=dw.ROW_BASE)
    replay_off = dw.OFFSET + 6
    off.fill_(replay_off - 1)
    graph.replay()
    torch.cuda.synchronize()
    got = {f: getattr(out, f).clone() for f in FIELDS}
    want = dynamic(sd, tl, tok, pd, c.proc, replay_off, dw.ROW_BASE, D)
    for f in FIELDS:
        assert same(got[f].cpu(), getattr(want, f)), f
    assert not all(same(got[f], want0[f]) for f in FIELDS)


def test_torch_op_equals_ops_verify_tree_dynamic(sd):
    c = dw.case("irregular64", 2049, torch.bfloat16, "multinomial")
    tl, tok = c.tl.to(DEV), c.tok.to(DEV)
    depth = max(tw.node_depths(c.parent))
    pd = parents_dev([c.parent] * c.B)
    stops = torch.tensor([int(c.tok[2, 0])], dtype=torch.long, device=DEV)
    want = sd.ops.verify_tree_dynamic(tl, tok, pd, spec_of(sd, c.proc), sd.PhiloxNoise(seed=dw.SEED, offset=dw.OFFSET), depth,
                                      stop_tokens=stops, row_base=dw.ROW_BASE)
    got = torch.ops.specdec.verify_tree_dynamic(tl, tok, pd, depth, stops, sd.ops.KIND[c.proc.kind], c.proc.temperature,
                                                c.proc.top_k, c.proc.top_p, dw.SEED, dw.OFFSET, dw.ROW_BASE)
    for g, f in zip(got, sd.ops.TREE_FIELDS + ("path",)):
        w = getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, f
        assert same(g, w), f


def test_argument_errors(sd):
    from specdec_amd.noise import StreamNoise
    tl = torch.zeros(1, 3, 64, device=DEV)
    tok = torch.zeros(1, 2, dtype=torch.long, device=DEV)
    pd = parents_dev([[-1, 0]])
    spec = sd.ops.ProcSpec("multinomial", 1.0)
    with pytest.raises(ValueError):
        sd.ops.verify_tree_dynamic(tl, tok, pd, spec, sd.PhiloxNoise(seed=1, offset=0), 0)
    with pytest.raises(ValueError):
        sd.ops.verify_tree_dynamic(tl, tok, pd, spec, sd.PhiloxNoise(seed=1, offset=0), 33)
    with pytest.raises(ValueError):
        sd.ops.verify_tree_dynamic(tl, tok, pd.long(), spec, sd.PhiloxNoise(seed=1, offset=0), 2)
    with pytest.raises(TypeError):
        sd.ops.verify_tree_dynamic(tl, tok, pd, spec, StreamNoise(), 2)
