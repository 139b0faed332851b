"""GPU tests of tree attention inside a model (specdec_amd.tree_attention) on a random-init
bf16 Llama (2 layers, hidden 256, 4 query heads, 2 K/V heads, D = 64, vocabulary 512): one cached tree
forward through the kernel against the loop's dense-mask path, and the cached loop with
attention="kernel".  The yardstick is never the code under test: it is the difference between the stock
"sdpa" and the stock "eager" attention on the same inputs, times 4 (three independently rounded bf16
pipelines over two layers are compared), or eps * max|value| if that is larger."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = torch.finfo(torch.bfloat16).eps


def _llama(seed, noise_of=None):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512)
    cfg._attn_implementation = "eager"
    torch.manual_seed(seed)
    model = LlamaForCausalLM(cfg).eval()
    if noise_of is not None:                                  # a drafter that agrees with its target often, not always
        model.load_state_dict(noise_of.state_dict())
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p) * 0.002)
    return model.to(DEV, torch.bfloat16)


@pytest.fixture(scope="module")
def target():
    pytest.importorskip("transformers")
    return _llama(1)


def _bound(a, b, scale):
    """4 x the stock implementations' difference, or eps * max|value|."""
    return max(4 * float((a.float() - b.float()).abs().max()), EPS * float(scale.float().abs().max()))


def _tree_forward(model, tokens, attention, stock):
    """Logits of a cached tree forward: 40 cached tokens, then 3 catch-up tokens and the tree's 28 nodes."""
    from specdec_amd.sampling.tree_decoding import _CachedModel
    from specdec_amd.tree import TokenTree
    tr = TokenTree.from_branching([4, 2, 1, 1])
    N = tr.num_nodes
    model.config._attn_implementation = stock
    cm = _CachedModel(model, torch.bfloat16, None, DEV, attention)
    with torch.no_grad():
        cm.forward(tokens[:, :40])
        allow, pos = cm.rows_of(tr, 43, 40, list(range(N)), list(range(N)))
        return cm.forward(tokens[:, 40:43 + N], allow, pos)


def test_one_cached_tree_forward_on_the_kernel(target):
    from specdec_amd import tree_attention
    tokens = torch.randint(0, 512, (1, 43 + 28), generator=torch.Generator().manual_seed(5)).to(DEV)
    eager = _tree_forward(target, tokens, "mask", "eager")
    sdpa = _tree_forward(target, tokens, "mask", "sdpa")
    before = dict(tree_attention.counts)
    got = _tree_forward(target, tokens, "kernel", "eager")
    assert tree_attention.counts["kernel"] == before["kernel"] + 2     # both layers of the tree forward
    assert target.config._attn_implementation == "eager"               # switched back
    yard, diff = float((sdpa.float() - eager.float()).abs().max()), float((got.float() - eager.float()).abs().max())
    bound = _bound(sdpa, eager, eager)
    print(f"[tree-attn-model] sdpa vs eager {yard:.3g}, kernel vs eager {diff:.3g}, bound {bound:.3g}")
    assert torch.isfinite(got).all() and diff <= bound


def test_a_forward_of_more_than_128_rows_falls_back_to_the_dense_mask(target):
    from specdec_amd import tree_attention
    from specdec_amd.sampling.tree_decoding import _CachedModel
    from specdec_amd.tree import TokenTree
    tokens = torch.randint(0, 512, (1, 130), generator=torch.Generator().manual_seed(6)).to(DEV)
    cm = _CachedModel(target, torch.bfloat16, None, DEV, "kernel")
    allow, pos = cm.rows_of(TokenTree([-1]), 130, 0, [], [])           # 130 causal catch-up rows
    before = dict(tree_attention.counts)
    with torch.no_grad():
        got = cm.forward(tokens, allow, pos)
        want = target(input_ids=tokens).logits[0]
    assert tree_attention.counts == before
    assert float((got.float() - want.float()).abs().max()) <= 4 * EPS * float(want.float().abs().max())


class Spy:
    """A model as the loop sees it; remembers the cache of its last forward."""

    def __init__(self, model):
        self.model, self.config, self.device, self.dtype = model, model.config, model.device, model.dtype

    def __call__(self, **kw):
        out = self.model(**kw)
        self.cache = out.past_key_values
        return out


def _plain_kv(model, ids, stock):
    model.config._attn_implementation = stock
    with torch.no_grad():
        cache = model(input_ids=ids, use_cache=True).past_key_values
    model.config._attn_implementation = "eager"
    return torch.stack([torch.stack([layer.keys, layer.values]) for layer in cache.layers])


@pytest.mark.parametrize("static", [False, True], ids=["dynamic", "static"])
def test_the_kernel_loop_leaves_the_committed_tokens_in_the_target_cache(target, static):
    """A wrong descriptor moves cache entries by O(1); the stock implementations differ by bf16 roundings."""
    from specdec_amd import tree_attention
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.tree import TokenTree
    prompt, spy, trace = [5, 17, 99, 3, 250, 41], Spy(target), []
    before = tree_attention.counts["kernel"]
    tokens, _ = tree_speculative_generate(prompt, _llama(2, noise_of=target), spy, max_gen_len=24, eos_tokens_id=[-1],
                                          tree=TokenTree.from_branching([2, 2, 1]), use_cache=True, static_cache=static,
                                          children="topk", attention="kernel", trace=trace)
    assert len(tokens) == 24 and tree_attention.counts["kernel"] > before
    length = trace[-1]["cur"] + trace[-1]["n"]                          # committed positions of the last compaction
    ids = torch.tensor([(prompt + tokens)[:length]], device=DEV)
    got = torch.stack([torch.stack([layer.keys[:, :, :length], layer.values[:, :, :length]]) for layer in spy.cache.layers])
    eager, sdpa = _plain_kv(target, ids, "eager"), _plain_kv(target, ids, "sdpa")
    diff, bound = float((got.float() - eager.float()).abs().max()), _bound(sdpa, eager, eager)
    print(f"[tree-attn-model] loop {'static' if static else 'dynamic'}: cache vs plain forward {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
