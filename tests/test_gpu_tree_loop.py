"""GPU tests of the tree decoding loop (sampling/tree_decoding.py) on a FakeLM pair that honours
position_ids and checks the 4-D mask it is handed: every traced step replayed by the host model
(tests/tree_ref.py) on the step's Philox offset, the stop token, the refused cache and determinism."""
from types import SimpleNamespace

import pytest
import torch

import fakelm
import multi_walk as mw
import tree_ref as tref
import tree_walk as tw
from test_gpu_tree import check_draw

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOOP_V, LOOP_TOKENS = 4096, 48
PROMPT = [5, 17, 101, 9, 2000, 77]
BRANCHING = [2, 2, 1]


class TreeFakeLM(fakelm.FakeLM):
    """FakeLM whose row is picked by (token, position_ids), as a model under a tree mask needs.  Every
    call's 4-D mask must be the loop's tree's (possibly truncated to a depth, over its first n nodes)
    with the matching position_ids; `calls` records (sequence length, n)."""

    def __init__(self, bank, tree, **kw):
        super().__init__(bank, **kw)
        self.tree = tree
        self.calls = []

    def __call__(self, input_ids=None, attention_mask=None, position_ids=None, use_cache=False, **_):
        ids = input_ids.to(self.bank.device)
        B, L = ids.shape
        if attention_mask is None:                                    # a plain causal forward (the first token)
            position_ids = torch.arange(L, device=ids.device)[None]
            self.calls.append((L, None))
        else:
            assert attention_mask.shape == (1, 1, L, L) and attention_mask.is_floating_point()
            assert position_ids is not None and position_ids.shape == (1, L)
            found = None
            for depth in range(self.tree.depth, 0, -1):
                tr = self.tree.truncated(depth)
                for n in range(0, min(tr.num_nodes, L - 1) + 1):     # the fewest nodes: a causal mask is n = 0
                    mask, pos = tr.attention_inputs(L - n, attention_mask.dtype, ids.device, num_nodes=n)
                    if torch.equal(mask, attention_mask) and torch.equal(pos, position_ids):
                        found = (depth, n)
                        break
                if found:
                    break
            assert found is not None, "the mask is not the ancestor mask of the loop's tree"
            self.calls.append((L, found[1]))
        idx = (ids * 31 + position_ids.to(ids.device) * self.pos_mult) % self.bank.shape[0]
        return SimpleNamespace(logits=self.bank[idx], past_key_values=None)


@pytest.fixture(scope="module")
def pair():
    from specdec_amd.tree import TokenTree
    tree = TokenTree.from_branching(BRANCHING)
    t, d = fakelm.make_banks(LOOP_V, sigma=1.0)
    return TreeFakeLM(t.to(DEV), tree), TreeFakeLM(d.to(DEV), tree), tree


def _loop_seed(s):
    """The PhiloxNoise seed the loop draws from torch's generator after torch.manual_seed(s)."""
    torch.manual_seed(s)
    return int(torch.randint(0, 2 ** 62, (1,)).item()) & 0xFFFFFFFFFFFFFFFF


def _generate(pair, seed, eos=(LOOP_V + 5,), **kw):
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter, tree = pair
    target.calls.clear()
    drafter.calls.clear()
    torch.manual_seed(seed)
    kw.setdefault("max_gen_len", LOOP_TOKENS)
    return tree_speculative_generate(PROMPT, drafter, target, logits_processor=MultinomialProcessor(1.0),
                                     eos_tokens_id=list(eos), tree=tree, **kw)


def _bank_row(lm, token, position):
    return lm.bank[(int(token) * 31 + int(position) * lm.pos_mult) % lm.bank.shape[0]].cpu()


def test_loop_steps_equal_the_host_model(pair):
    target, drafter, tree = pair
    s, trace = 3, []
    toks, rate = _generate(pair, s, trace=trace)
    seq = PROMPT + toks
    assert len(toks) == LOOP_TOKENS and 0 < rate < 1 and len(trace) >= LOOP_TOKENS // (tree.depth + 1)
    seed, proc = _loop_seed(s), mw.PROCS["multinomial"]
    close = 0
    for st in trace:
        cur, parent, tok = st["cur"], st["parent"], st["draft_tokens"].numpy()
        depths = tw.node_depths(parent)
        at = [seq[cur - 1]] + tok.tolist()
        pos = [cur - 1] + [cur - 1 + d for d in depths]
        P, Q = mw.bank_rows(target, at, pos, proc), mw.bank_rows(drafter, at, pos, proc)
        r = tref.philox_step(P, Q, tok, parent, seed, st["offset"], 0)
        got, want = (st["n"], st["path"], st["sibling_rejects"]), (r.n, r.path, r.rejects)
        print(f"[tree-loop] step cur={cur} N={len(parent)} got={got} want={want} close={r.close}")
        if got != want:
            assert r.close, (cur, got, want)
            close += 1
        assert seq[cur:cur + st["n"]] == [int(tok[c]) for c in st["path"]] and seq[cur + st["n"]] == st["x"]
        if got == want:
            slot = r.mass_at if r.status == tref.RESIDUAL else r.slot
            slack = 1e-5 + mw.flip_slack(_bank_row(target, at[slot], pos[slot]), target.bank.dtype)
            if r.status == tref.RESIDUAL:
                slack += mw.flip_slack(_bank_row(drafter, at[slot], pos[slot]), drafter.bank.dtype)
            assert r.weights[st["x"]] > 0
            check_draw(f"step cur={cur}", r, st["x"], slack)
    assert close <= 1
    assert sum(st["n"] for st in trace) / sum(max(tw.node_depths(st["parent"])) for st in trace) == pytest.approx(rate)
    # the target ran one plain forward (the first token), then one tree-masked forward over the whole tree per step;
    # the drafter one forward per level over prefix + the nodes of the levels before it
    assert target.calls[0] == (len(PROMPT), None)
    assert target.calls[1:len(trace) + 1] == [(st["cur"] + len(st["parent"]), len(st["parent"])) for st in trace]
    want_d = []
    for st in trace:
        depths = tw.node_depths(st["parent"])
        for d in range(max(depths)):
            n = sum(x <= d for x in depths)
            want_d.append((st["cur"] + n, n))
    assert drafter.calls[:len(want_d)] == want_d
    # the tree is truncated to the depth that still fits before the sampled token
    for st in trace:
        assert st["parent"] == tree.truncated(min(tree.depth, len(seq) - st["cur"] - 1)).parent
    short = []
    toks, _ = _generate(pair, s, trace=short, max_gen_len=3)        # one position left after the first token's draft
    assert len(toks) == 3 and short[0]["parent"] == [-1, -1]


def test_loop_ends_at_a_stop_token(pair):
    target = pair[0]
    stops = fakelm.likely_tokens(target)
    toks, _ = _generate(pair, 5, eos=stops)
    assert 0 < len(toks) < LOOP_TOKENS and toks[-1] in stops and not any(t in stops for t in toks[:-1])


def test_loop_is_deterministic_under_manual_seed(pair):
    a = _generate(pair, 21)
    b = _generate(pair, 21)
    c = _generate(pair, 22)
    assert a == b and a[0] != c[0]


def test_a_cache_and_a_user_processor_are_refused(pair):
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter, tree = pair
    with pytest.raises(ValueError, match="Unsupported cache type."):
        _generate(pair, 1, use_cache=True)

    class Mine(MultinomialProcessor):
        def _process(self, logits):
            return logits

    with pytest.raises(TypeError):
        tree_speculative_generate(PROMPT, drafter, target, logits_processor=Mine(1.0), tree=tree)
