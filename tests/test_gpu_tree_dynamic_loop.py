"""GPU tests of the dynamic-tree decoding loop (sampling/dynamic_tree_decoding.py) on the tiny fp32 Llamas
of tests/test_gpu_tree_cached_loop.py: greedy output equal to the target's own greedy decode for several
DynamicTreeSpecs and sequence ends, full acceptance when the drafter is the target, every traced step
of a stochastic run replayed by the host model (the target's rows recomputed under
TokenTree.attention_inputs of the traced parents, tests/tree_distinct_ref.py's walk on the numpy Philox),
and stop tokens."""
import numpy as np
import pytest
import torch

import multi_walk as mw
import tree_distinct_ref as dref
import tree_dynamic_ref as yref
from oracle import specdec_ref as ref
from test_gpu_tree import check_draw
from test_gpu_tree_cached_loop import GEN, PROMPT, TEMPERATURE, _tiny_llama
from test_gpu_tree_loop import _loop_seed
from tree_ref import children_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPECS = [(1, 1, 1, 1), (4, 2, 2, 8), (5, 8, 8, 64)]


@pytest.fixture(scope="module")
def models():
    pytest.importorskip("transformers")
    target = _tiny_llama(1).to(DEV)
    return target, _tiny_llama(2, noise_of=target).to(DEV)


@pytest.fixture(scope="module")
def greedy_decode(models):
    from specdec_amd.sampling.base_decoding import autoregressive_generate
    return autoregressive_generate(PROMPT, models[0], max_gen_len=GEN, eos_tokens_id=[-1])


def _generate(target, drafter, spec, seed=11, eos=(-1,), proc=None, **kw):
    from specdec_amd.sampling import dynamic_tree_speculative_generate
    from specdec_amd.tree import DynamicTreeSpec
    from specdec_amd.utils.logits_processor import GreedyProcessor
    torch.manual_seed(seed)
    kw.setdefault("max_gen_len", GEN)
    return dynamic_tree_speculative_generate(PROMPT, drafter, target, logits_processor=proc or GreedyProcessor(),
                                             eos_tokens_id=list(eos), spec=DynamicTreeSpec(*spec), **kw)


def _check_tree(st, spec, total_len):
    """What the verify's ABI asks of a traced tree, and the truncation near the end of the sequence."""
    L, W, c, N = spec
    parent, depth = st["parent"], st["depth"]
    levels = min(L, total_len - st["cur"] - 1)
    F, base = yref.shape(levels, W, c)
    assert len(parent) == min(N, base[-1])
    assert all(-1 <= p < i for i, p in enumerate(parent))
    assert max(len(k) for k in children_of(parent)) <= c and max(depth) <= levels
    assert depth == [1 if p < 0 else depth[p] + 1 for p in parent]
    toks = st["draft_tokens"].tolist()
    assert all(len({toks[k] for k in ks}) == len(ks) for ks in children_of(parent))     # distinct children
    return levels


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "L%d-W%d-c%d-N%d" % s)
def test_greedy_loop_emits_the_targets_greedy_decode(models, greedy_decode, spec):
    target, drafter = models
    trace = []
    toks, rate = _generate(target, drafter, spec, trace=trace)
    assert toks == greedy_decode and len(toks) == GEN
    seen = {_check_tree(st, spec, len(PROMPT) + GEN) for st in trace}
    print(f"[dynamic-loop] spec {spec}: rate {rate:.3f}, steps {len(trace)}, levels seen {sorted(seen)}")
    assert max(seen) == spec[0] and rate > 0
    assert sum(st["n"] for st in trace) / sum(_check_tree(st, spec, len(PROMPT) + GEN) for st in trace) == pytest.approx(rate)
    with torch.no_grad():                                  # the claim needs unique row maxima
        seq = torch.tensor([PROMPT + toks], device=DEV)
        top2 = torch.topk(target(input_ids=seq).logits[0].float(), 2, dim=-1).values
    assert bool((top2[:, 0] > top2[:, 1]).all())


@pytest.mark.parametrize("gen", [1, 2, 3, 7])
def test_sequence_ends_truncate_the_tree(models, greedy_decode, gen):
    """max_gen_len 1: the first token alone; 2: no room for a draft (a plain step); 3, 7: levels and
    num_nodes shrink to what fits before the sampled token."""
    target, drafter = models
    trace = []
    toks, _ = _generate(target, drafter, (5, 8, 8, 64), max_gen_len=gen, trace=trace)
    assert toks == greedy_decode[:gen]
    total = len(PROMPT) + gen
    levels = [_check_tree(st, (5, 8, 8, 64), total) for st in trace]
    assert all(lv == min(5, total - st["cur"] - 1) for lv, st in zip(levels, trace))
    if gen <= 2:
        assert trace == []
    if gen == 3:
        assert levels[0] == 1 and len(trace[0]["parent"]) == 8
    # first_target=False: the loop starts with a tree step
    toks2, _ = _generate(target, drafter, (4, 2, 2, 8), max_gen_len=gen, first_target=False)
    assert toks2 == greedy_decode[:gen]


def test_the_target_as_its_own_drafter_accepts_every_full_step(models, greedy_decode):
    target = models[0]
    trace = []
    toks, rate = _generate(target, target, (4, 1, 1, 4), trace=trace)
    assert toks == greedy_decode
    full = [st for st in trace if len(st["parent"]) == 4]
    assert len(full) >= 4 and all(st["n"] == 4 and st["path"] == [0, 1, 2, 3] for st in full)
    assert all(st["parent"] == list(range(-1, len(st["parent"]) - 1)) for st in trace)
    print(f"[dynamic-loop] self-drafting: rate {rate:.3f} over {len(trace)} steps")


def test_stochastic_steps_equal_the_host_model(models):
    from specdec_amd.tree import TokenTree
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = models
    s, spec = 5, (4, 4, 3, 16)
    trace = []
    toks, rate = _generate(target, drafter, spec, seed=s, proc=MultinomialProcessor(temperature=TEMPERATURE), trace=trace)
    seq = PROMPT + toks
    assert len(toks) == GEN and len(trace) >= 3
    seed, proc = _loop_seed(s), ref.Processor("multinomial", TEMPERATURE)
    close = 0
    for st in trace:
        cur, parent, tok = st["cur"], st["parent"], st["draft_tokens"].numpy()
        _check_tree(st, spec, len(seq))
        N = len(parent)
        with torch.no_grad():                              # the target's rows under the traced topology's own mask
            mask, pos = TokenTree(parent).attention_inputs(cur, torch.float32, DEV)
            ids = torch.tensor([seq[:cur] + tok.tolist()], device=DEV)
            tl = target(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=False).logits[0, cur - 1:cur + N].cpu()
        P = ref.process(tl, proc, exact=True).double().numpy()
        r = dref.philox_step(P, tok, parent, seed, st["offset"], 0)
        got, want = (st["n"], st["path"], st["sibling_rejects"]), (r.n, r.path, r.rejects)
        print(f"[dynamic-loop] step cur={cur} N={N} got={got} want={want} close={r.close} x={st['x']} host_x={r.x}")
        if got != want:
            assert r.close, (cur, got, want)
            close += 1
            continue
        assert seq[cur:cur + st["n"]] == [int(tok[k]) for k in st["path"]] and seq[cur + st["n"]] == st["x"]
        assert r.weights[st["x"]] > 0
        check_draw(f"step cur={cur}", r, st["x"], 1e-5 + mw.flip_slack(tl[r.slot] / TEMPERATURE, torch.float32))
    assert close <= 1
    assert 0 < rate <= 1 and any(st["n"] >= 1 for st in trace)
    # deterministic under the seed, different under another
    again, _ = _generate(target, drafter, spec, seed=s, proc=MultinomialProcessor(temperature=TEMPERATURE))
    assert again == toks


def test_a_stop_token_on_the_path_ends_the_loop_as_in_the_tree_loop(models, greedy_decode):
    from specdec_amd.sampling import tree_speculative_generate
    from specdec_amd.tree import TokenTree
    target, drafter = models
    trace = []
    _generate(target, drafter, (4, 2, 2, 8), trace=trace)
    st = next(st for st in trace if st["n"] >= 2)
    stop = int(st["draft_tokens"][st["path"][1]])           # accepted in mid-path
    want = greedy_decode[:greedy_decode.index(stop) + 1]
    toks, _ = _generate(target, drafter, (4, 2, 2, 8), eos=[999999, stop])
    assert toks == want and toks[-1] == stop
    torch.manual_seed(11)
    ref_toks, _ = tree_speculative_generate(PROMPT, drafter, target, max_gen_len=GEN, eos_tokens_id=[999999, stop],
                                            tree=TokenTree.from_branching([2, 2, 1, 1]), children="topk")
    assert toks == ref_toks


def test_spec_tuples_and_the_default_spec(models, greedy_decode):
    from specdec_amd.sampling import dynamic_tree_speculative_generate
    target, drafter = models
    torch.manual_seed(1)
    a, _ = dynamic_tree_speculative_generate(PROMPT, drafter, target, gamma=3, max_gen_len=GEN, eos_tokens_id=[-1])
    torch.manual_seed(1)
    b, _ = dynamic_tree_speculative_generate(PROMPT, drafter, target, spec=(3, 1, 1, 3), max_gen_len=GEN, eos_tokens_id=[-1])
    assert a == b == greedy_decode
    assert np.all(np.array(a) >= 0)
