"""GPU tests of the cached tree loop (tree_speculative_generate(use_cache=True)) on tiny
fp32 Llamas (vocab 512, 2 layers, eager attention): the tokens equal the uncached loop's, the caches
hold the committed tokens' K/V after every compaction, every forward feeds only what its cache lacks,
a stop token on the path ends the loop alike, and an unknown cache type is refused.

Every loop runs once (the module fixture) and the tests read its record."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROMPT = [5, 17, 99, 3, 250, 41]
GEN = 30
TREES = {"b221": [-1, -1, 0, 0, 1, 1, 2, 3, 4, 5],       # TokenTree.from_branching([2, 2, 1])
         "unordered": [-1, 0, -1, 2, 0]}                  # node indices not level-ordered: levels [0, 2], [1, 3, 4]
PROCS = ("greedy", "multinomial")
KINDS = {"dynamic": dict(use_cache=True), "static": dict(use_cache=True, static_cache=True)}
SEED = 11
NOISE, TEMPERATURE = 0.002, 0.1     # the drafter's weight noise; the multinomial processor's temperature


def _tiny_llama(seed, noise_of=None):
    """test_gpu_window._tiny_llama's shape with eager attention.  noise_of: a model whose weights this one
    copies and perturbs slightly — a drafter that agrees with its target often, not always."""
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=256)
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).eval()
    if noise_of is not None:
        model.load_state_dict(noise_of.state_dict())
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p) * NOISE)
    return model


class Recorder:
    """A model as the loop sees it; records per call the tokens fed and, when a cache comes in, a copy of
    its K/V tensors as they are BEFORE the call (what the compaction before it left)."""

    def __init__(self, model):
        self.model, self.config = model, model.config
        self.device, self.dtype = model.device, model.dtype
        self.fed, self.before = [], []

    def __call__(self, **kw):
        cache = kw.get("past_key_values")
        self.fed.append(kw["input_ids"].shape[1])
        layers = getattr(cache, "layers", None) or []
        self.before.append([(layer.keys.clone(), layer.values.clone()) for layer in layers
                            if getattr(layer, "keys", None) is not None and torch.is_tensor(layer.keys)])
        return self.model(**kw)


def _proc(name):
    from specdec_amd.utils.logits_processor import GreedyProcessor, MultinomialProcessor
    return GreedyProcessor() if name == "greedy" else MultinomialProcessor(temperature=TEMPERATURE)


def _generate(target, drafter, tree, proc, seed=SEED, eos=(-1,), **kw):
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.tree import TokenTree
    torch.manual_seed(seed)
    return tree_speculative_generate(PROMPT, drafter, target, logits_processor=_proc(proc), max_gen_len=GEN,
                                     eos_tokens_id=list(eos), tree=TokenTree(TREES[tree]), **kw)


@pytest.fixture(scope="module")
def models():
    pytest.importorskip("transformers")
    target = _tiny_llama(1).to(DEV)
    return target, _tiny_llama(2, noise_of=target).to(DEV)


@pytest.fixture(scope="module")
def runs(models):
    """{(tree, proc): {"uncached": (tokens, rate), kind: SimpleNamespace(tokens, rate, trace, target, drafter)}}"""
    out = {}
    for tree in TREES:
        for proc in PROCS:
            rec = {"uncached": _generate(*models, tree, proc)}
            for kind, kw in KINDS.items():
                t, d, trace = Recorder(models[0]), Recorder(models[1]), []
                tokens, rate = _generate(t, d, tree, proc, trace=trace, **kw)
                rec[kind] = SimpleNamespace(tokens=tokens, rate=rate, trace=trace, target=t, drafter=d)
            out[tree, proc] = rec
    return out


# ---------------------------------------------------------------- tokens
@pytest.mark.parametrize("proc", PROCS)
@pytest.mark.parametrize("tree", list(TREES))
def test_cached_loops_emit_the_uncached_loops_tokens(runs, tree, proc):
    """Under one torch.manual_seed the DynamicCache loop, the StaticCache loop and the uncached loop draw
    from the same Philox stream, so tokens and acceptance rate are equal (the precedent:
    test_static_cache_device_crop_equals_the_uncached_loop).  On the parent commit use_cache=True raises."""
    rec = runs[tree, proc]
    tokens, rate = rec["uncached"]
    assert len(tokens) == GEN
    for kind in KINDS:
        print(f"[tree-cached] {tree} {proc} {kind}: rate {rec[kind].rate:.3f}, n per step {[s['n'] for s in rec[kind].trace]}")
        assert rec[kind].tokens == tokens, kind
        assert rec[kind].rate == rate, kind


def test_the_drafter_gets_paths_accepted(runs):
    """The record the other tests read is no trivial one: in every tree some step accepts a full path (whose
    last node the drafter never fed), some step accepts less, and some accepted node lies above its depth's
    position, so the compaction moves real entries.  (Random-init logits are nearly flat: the drafter is the
    target plus weight noise of a tenth of the init scale, and the multinomial runs at temperature 0.1.)"""
    for tree in TREES:
        steps = [s for proc in PROCS for s in runs[tree, proc]["dynamic"].trace]
        depth = 3 if tree == "b221" else 2
        seen = {s["n"] for s in steps if len(s["parent"]) == len(TREES[tree])}
        assert depth in seen and min(seen) < depth, (tree, seen)
        assert any(s["path"] != list(range(len(s["path"]))) for s in steps), tree


# ---------------------------------------------------------------- forward sizes and the length bookkeeping
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("proc", PROCS)
@pytest.mark.parametrize("tree", list(TREES))
def test_every_forward_feeds_only_what_its_cache_lacks(runs, tree, proc, kind):
    from specdec_amd.tree import TokenTree
    r = runs[tree, proc][kind]
    assert r.target.fed[0] == len(PROMPT)                                   # the plain first-token forward
    t_calls, d_calls = r.target.fed[1:], list(r.drafter.fed)
    for i, st in enumerate(r.trace):
        tr = TokenTree(st["parent"])
        assert st["cache_len_target"] == st["cur"] - 1
        assert t_calls[i] == 1 + tr.num_nodes                               # the root and the N nodes
        level1 = d_calls.pop(0)
        assert level1 == st["cur"] - st["cache_len_drafter"]
        assert level1 == (len(PROMPT) + 1 if i == 0 else level1) and (i == 0 or level1 in (1, 2))   # x; before it the last node of a full path
        for k in range(1, tr.depth):
            assert d_calls.pop(0) == len(tr.levels[k - 1])                  # the nodes of the level before
        if i > 0:
            prev = r.trace[i - 1]
            depth = TokenTree(prev["parent"]).depth
            assert st["cache_len_drafter"] == prev["cur"] + min(prev["n"], depth - 1)
    assert not d_calls and all(n == 1 for n in t_calls[len(r.trace):])      # then only plain tail steps


# ---------------------------------------------------------------- cache contents
def _kv(model, ids):
    """K/V [layers][2] of a plain causal cached forward over `ids` [1, L]."""
    with torch.no_grad():
        cache = model(input_ids=ids, use_cache=True).past_key_values
    return [(layer.keys, layer.values) for layer in cache.layers]


def _kv_err(got, want, length):
    """Largest |difference| of the first `length` positions, over layers and over K and V."""
    return max(float((g[:, :, :length] - w[:, :, :length]).abs().max()) for gl, wl in zip(got, want) for g, w in zip(gl, wl))


def _tree_vs_plain(model, tree_parent):
    """The measurement that sets the tolerance, with no compaction involved: a cached tree forward's K/V
    entries along a chosen path (the last leaf's) against a plain causal cached forward over the same
    tokens.  Returns (difference, the same difference with the path's first node swapped for a sibling)."""
    from specdec_amd.sampling.tree_decoding import _allowed
    from specdec_amd.tree import TokenTree
    tree = TokenTree(tree_parent)
    N, P = tree.num_nodes, len(PROMPT)
    prefix = torch.tensor([PROMPT], device=DEV)
    nodes = torch.tensor([[100 + 7 * i for i in range(N)]], device=DEV)
    path = tree.path_to(N - 1)
    sibling = next(c for c in tree.children[0] if c != path[0])
    allow, pos = _allowed(tree, P, P - 1, list(range(N)), list(range(N)))
    mask = torch.zeros(allow.shape, dtype=torch.float32).masked_fill_(~allow, torch.finfo(torch.float32).min)
    with torch.no_grad():
        cache = model(input_ids=prefix[:, :P - 1], use_cache=True).past_key_values
        cache = model(input_ids=torch.cat([prefix[:, P - 1:], nodes], 1), attention_mask=mask[None, None].to(DEV),
                      position_ids=pos.to(DEV), past_key_values=cache, use_cache=True).past_key_values
        plain = model(input_ids=prefix[:, :P - 1], use_cache=True).past_key_values
        plain = model(input_ids=torch.cat([prefix[:, P - 1:], nodes[:, path]], 1), past_key_values=plain,
                      use_cache=True).past_key_values

    def diff(p):
        at = torch.tensor(list(range(P)) + [P + i for i in p], device=DEV)
        got = [(layer.keys.index_select(2, at), layer.values.index_select(2, at)) for layer in cache.layers]
        want = [(layer.keys, layer.values) for layer in plain.layers]
        return _kv_err(got, want, P + len(p))
    return diff(path), diff([sibling] + path[1:])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("tree", list(TREES))
def test_caches_hold_the_committed_tokens_after_every_compaction(runs, models, tree, kind):
    """Before every step's first forward — that is, after the compaction of the step before — each cache's
    K/V on [0, cache_len) equals the K/V of ONE plain causal cached forward over the final sequence
    (causal: its prefix of any length is the forward over the tokens committed by then).

    Tolerance: 10x the largest K/V difference between a cached tree forward's entries along a path and
    the plain causal cached forward over the same tokens, measured here with no compaction involved
    (fp32 GEMMs of other shapes and another mask; nobody can guess that figure).  A wrong slot moves an
    entry by the scale of the K/V values themselves: the same measurement with the path's first node
    swapped for its sibling must fail the tolerance by far.  Measured on an MI355X: difference 1.2e-7 to
    2.4e-7, with the sibling 0.89 to 0.93, largest error after a compaction 4.6e-7."""
    from specdec_amd.tree import TokenTree
    worst, tols = 0.0, {}
    for which, model in (("target", models[0]), ("drafter", models[1])):
        measured, swapped = _tree_vs_plain(model, TREES[tree])
        tols[which] = 10 * measured
        print(f"[tree-cached] {tree} {kind} {which}: tree-vs-plain K/V difference {measured:.3g} "
              f"(tolerance {tols[which]:.3g}); with a sibling swapped in {swapped:.3g}")
        assert swapped > 100 * tols[which] and swapped > 1e-3
    for proc in PROCS:
        r = runs[tree, proc][kind]
        seq = torch.tensor([PROMPT + r.tokens], device=DEV)
        for which, model, rec in (("target", models[0], r.target), ("drafter", models[1], r.drafter)):
            tol = tols[which]
            want = _kv(model, seq)
            call = 1 if which == "target" else 0                            # the target's call 0 is the first token's
            for st in r.trace:
                length = st[f"cache_len_{which}"]
                got = rec.before[call]
                if length:                                                  # the drafter's first forward starts empty
                    assert got and got[0][0].shape[2] >= length
                    if kind == "dynamic":
                        assert got[0][0].shape[2] == length
                    err = _kv_err(got, want, length)
                    worst = max(worst, err)
                    assert err <= tol, (which, proc, st["cur"], err, tol)
                call += 1 if which == "target" else TokenTree(st["parent"]).depth
    print(f"[tree-cached] {tree} {kind}: largest K/V error after a compaction {worst:.3g}")


# ---------------------------------------------------------------- the stop token, the refusal
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_stop_token_on_the_path_ends_the_loop_like_the_uncached_one(runs, models, kind):
    """A stop token that the loop is known to emit (the uncached run's 12th token, so a likely one): the
    cached and the uncached loop end at its first occurrence with the same tokens."""
    for tree in TREES:
        full = runs[tree, "multinomial"]["uncached"][0]
        stop = full[11]
        want = full[:full.index(stop) + 1]
        a, _ = _generate(*models, tree, "multinomial", eos=(stop,))
        b, _ = _generate(*models, tree, "multinomial", eos=(stop,), **KINDS[kind])
        assert a == want and b == want and len(want) < GEN


def test_an_unsupported_cache_object_is_refused(models):
    class StubCache:
        pass

    class StubModel(Recorder):
        def __call__(self, **kw):
            kw["past_key_values"] = None
            out = self.model(**kw)
            return SimpleNamespace(logits=out.logits, past_key_values=StubCache())

    with pytest.raises(ValueError, match="Unsupported cache type."):
        _generate(StubModel(models[0]), models[1], "b221", "greedy", use_cache=True)
    with pytest.raises(ValueError, match="Unsupported cache type."):
        _generate(models[0], StubModel(models[1]), "b221", "greedy", use_cache=True, first_target=False)
