"""block_speculative_generate on the GPU, on tests/fakelm.py pairs: every traced step recomputed by the
host model (tests/block_ref.py), γ = 1 against speculative_generate, cached against uncached decoding,
the stop on an eos, and the refusal of a user _process."""
import pytest
import torch

import block_cases as bc
import block_ref as br
import multi_walk as mw
import multidraft_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOOP_V, LOOP_G, LOOP_TOKENS = 4096, 4, 48
PROMPT = [5, 17, 101, 9, 2000, 77]


def _loop_seed(s):
    """The PhiloxNoise seed the loop draws from torch's generator after torch.manual_seed(s)."""
    torch.manual_seed(s)
    return int(torch.randint(0, 2 ** 62, (1,)).item()) & 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def pair():
    import fakelm
    return fakelm.make_pair(LOOP_V, sigma=1.0, device=DEV)


def _generate(pair, seed, gamma=LOOP_G, eos=(LOOP_V + 5,), **kw):
    from specdec_amd.sampling import block_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = pair
    torch.manual_seed(seed)
    return block_speculative_generate(PROMPT, drafter, target, gamma=gamma, logits_processor=MultinomialProcessor(1.0),
                                      max_gen_len=LOOP_TOKENS, eos_tokens_id=list(eos), **kw)


def _bank_row(lm, token, position):
    return lm.bank[(int(token) * 31 + int(position) * lm.pos_mult) % lm.bank.shape[0]].cpu()


def test_loop_steps_equal_the_host_model(pair):
    """Every traced step recomputed from the FakeLM banks by the host model: n exactly unless the step
    is close, the accepted drafts and the emitted token in place, the token inside the widened interval
    of the host's draw."""
    target, drafter = pair
    s = 3
    trace = []
    toks, rate = _generate(pair, s, trace=trace)
    seq = PROMPT + toks
    assert len(toks) == LOOP_TOKENS and 0 < rate <= 1 and len(trace) >= LOOP_TOKENS // (LOOP_G + 1)
    seed, proc = _loop_seed(s), mw.PROCS["multinomial"]
    close = rescued = 0
    for st in trace:
        cur, g, tok = st["cur"], st["g"], st["draft_tokens"].numpy()
        assert tok.shape == (g,)
        P, Q = bc.step_rows(target, drafter, seq[cur - 1], cur, tok, proc)
        at = [seq[cur - 1]] + tok.tolist()
        slack = lambda lm, d: mw.flip_slack(_bank_row(lm, at[d], cur - 1 + d), lm.bank.dtype)   # noqa: E731
        s_tol = [mref.MASS_TOL + slack(target, d) + slack(drafter, d) for d in range(g)]
        r = br.philox_step(P, Q, tok, seed, st["offset"], 0, s_tol=s_tol, bonus_tol=mref.MASS_TOL + slack(target, g))
        print(f"[block-loop] step cur={cur} g={g} n={st['n']} want={r.n} tokenwise={r.tokenwise_n} close={r.close}")
        assert seq[cur:cur + st["n"]] == tok[:st["n"]].tolist() and seq[cur + st["n"]] == st["x"]
        if r.close:
            close += 1
            continue
        assert st["n"] == r.n, (cur, st["n"], r.n)
        rescued += r.rescue
        assert r.weights[st["x"]] > 0
        assert mw.draw_excess(r, st["x"], r.draw_slack) <= 1.0, (cur, st["x"], r.x)
    assert close <= 1
    assert sum(st["n"] for st in trace) / sum(st["g"] for st in trace) == pytest.approx(rate)
    print(f"[block-loop] {len(trace)} steps, {rescued} rescued, rate {rate:.3f}")


def test_loop_with_one_draft_is_speculative_generate(pair):
    import specdec_amd
    from specdec_amd.sampling import speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = pair
    toks, rate = _generate(pair, 11, gamma=1)
    specdec_amd.set_noise_mode("philox", _loop_seed(11))
    try:
        want = speculative_generate(PROMPT, drafter, target, gamma=1, logits_processor=MultinomialProcessor(1.0),
                                    max_gen_len=LOOP_TOKENS, eos_tokens_id=[LOOP_V + 5])
    finally:
        specdec_amd.set_noise_mode("stream")
    assert (toks, rate) == want


def test_cached_loop_emits_the_uncached_tokens(pair):
    """use_cache crops the caches by the verify's prune outputs: the FakeLM's logits depend on the
    position, so a cache left too long or cut too short changes the tokens."""
    want = _generate(pair, 5)
    got = _generate(pair, 5, use_cache=True)
    assert got == want


def test_loop_stops_on_an_eos(pair):
    toks, _ = _generate(pair, 7)
    eos = toks[LOOP_TOKENS // 2]
    cut, _ = _generate(pair, 7, eos=(LOOP_V + 5, eos))
    assert cut == toks[:toks.index(eos) + 1]


def test_loop_refuses_a_user_process(pair):
    from specdec_amd.sampling import block_speculative_generate
    from specdec_amd.utils.logits_processor import MultinomialProcessor
    target, drafter = pair

    class Own(MultinomialProcessor):
        def _process(self, logits):
            return logits

    with pytest.raises(TypeError):
        block_speculative_generate(PROMPT, drafter, target, gamma=LOOP_G, logits_processor=Own(1.0))
