"""The host model of the device n-gram store's tables (tests/ngram_store_model.py) against the
oracle, and the bit layout of its keys.

The model applies each call as the kernels do: phase 1 over all records of the call in an arbitrary
(seeded) order, then phase 2 over all of them, with the keys earlier calls left in gram_best still
in place ("keys only grow").  The oracle applies the same records one by one in the reference's
order.  After every call the decoded best map and counts must be the oracle's."""
import random

import pytest

import ngram_store_model as m
from oracle import specdec_ref as ref

CONFIGS = [("one", 2), ("one", 3), ("one", 4), ("multi", 2), ("multi", 3), ("multi", 4)]


def _stream(kind, n, seed):
    """A mixed sequence of calls over few symbols: ("init", rows) with B > 1, ("update", rows, nexts)
    with k = 1..3; the update histories grow by the first next token, as in the decoding loops."""
    rng = random.Random(1000 * seed + 10 * n + len(kind))
    S = rng.randint(3, 6)
    B = rng.randint(2, 4)
    L =rng.randint(1, 12)
    hist = [[rng.randrange(S) for _ in range(L)] for _ in range(B)]
    calls = [("init", [list(h) for h in hist])]
    for _ in range(14):
        if rng.random() < 0.25:
            Bi, Li = rng.randint(2, 4), rng.randint(1, 10)
            calls.append(("init", [[rng.randrange(S) for _ in range(Li)] for _ in range(Bi)]))
        else:
            k = rng.randint(1, 3)
            nexts = [[rng.randrange(S) for _ in range(k)] for _ in range(B)]
            calls.append(("update", [list(h) for h in hist], nexts))
            for h, nx in zip(hist, nexts):
                h.append(nx[0])
    return calls


@pytest.mark.parametrize("kind,n", CONFIGS)
def test_model_equals_oracle_after_every_batch(kind, n):
    for seed in range(24):
        perm = random.Random(seed)
        model = m.StoreModel(kind, n, 1 << 10, 1 << 11)
        theirs = ref.NgramStore(kind, n, 8, ref.TorchNoise(None))
        n_rec = 0
        for c, call in enumerate(_stream(kind, n, seed)):
            if call[0] == "init":
                model.initialize(call[1], perm)
                for row in call[1]:
                    theirs.initialize(row)
            else:
                model.update(call[1], call[2], perm)
                for row, nx in zip(call[1], call[2]):
                    theirs.update(row, nx)
            grams, pairs, best = model.decoded()
            want_grams, want_counts, want_best = m.oracle_maps(theirs)
            assert grams == want_grams, (seed, c)
            assert {k: v[0] for k, v in pairs.items()} == want_counts, (seed, c)
            assert best == want_best, (seed, c)
            n_rec = sum(want_counts.values())
            assert model.n_valid == n_rec and sum(model.pair_count) == n_rec
        assert model.status == 0
        assert n_rec > 0 or (kind, n) == ("multi", 2)   # NGramStorage(2) has no order to record


def test_model_streams_are_tie_heavy_and_mixed():
    """The streams above do what they are meant to: several initialize calls with B > 1, updates
    with every k in 1..3, and grams whose top count is shared by two tokens."""
    kinds, ks, tie = set(), set(), False
    for seed in range(24):
        for call in _stream("one", 3, seed):
            kinds.add(call[0])
            assert len(call[1]) > 1
            if call[0] == "update":
                ks.add(len(call[2][0]))
        theirs = ref.NgramStore("one", 3, 8, ref.TorchNoise(None))
        for call in _stream("one", 3, seed):
            for b, row in enumerate(call[1]):
                theirs.initialize(row) if call[0] == "init" else theirs.update(row, call[2][b])
        for per in theirs.counts.get(2, {}).values():
            top = max(per.values())
            tie |= sum(1 for c in per.values() if c == top) > 1
    assert kinds == {"init", "update"} and ks == {1, 2, 3} and tie


EDGE_IDS = (0, 1, 1 << 16, (1 << 17) - 2, (1 << 17) - 1)


def test_gram_key_packing():
    seen = {}
    for level in (1, 2, 3):
        grams = [()]
        for _ in range(level):
            grams = [g + (t,) for g in grams for t in EDGE_IDS]
        for g in grams:
            k = m.gram_key(level, g)
            assert 0 <= k < 1 << 64 and k >> 63 == 1
            assert m.decode_gram_key(k) == (level, g)
            assert (k >> m.LEVEL_SHIFT) & 0xFFF == level           # t2 << 34 ends at bit 50
            assert k not in seen, (seen.get(k), (level, g))
            seen[k] = (level, g)
    assert len(seen) == 5 + 25 + 125
    # the largest id at the last position leaves the level field alone: its top bit is bit 50
    assert m.gram_key(3, (0, 0, m.TOK_MASK)) == m.USED | (3 << 51) | (m.TOK_MASK << 34)
    assert (m.TOK_MASK << 34).bit_length() == 51
    # the same ids at another level, and a level-j gram padded with id 0, are other keys
    assert m.gram_key(1, (0,)) != m.gram_key(2, (0, 0)) != m.gram_key(3, (0, 0, 0))


def test_pair_and_best_key_packing():
    for slot in (0, 1, (1 << 21) - 1, (1 << 40) - 1):
        for tok in EDGE_IDS:
            k = m.pair_key(slot, tok)
            assert k >> 63 == 1 and k < 1 << 64 and m.decode_pair_key(k) == (slot, tok)
    for count in (1, 2, m.COUNT_MAX - 1, m.COUNT_MAX):
        for ts in (0, 1, m.TS_MAX - 1, m.TS_MAX):
            for tok in EDGE_IDS:
                b = m.pack_best(count, ts, tok)
                assert 0 < b < 1 << 64 and m.unpack_best(b) == (count, ts, tok)
    # larger count first, then the earlier latest ts; the token never decides between two pairs
    assert m.pack_best(3, m.TS_MAX, 0) > m.pack_best(2, 0, m.TOK_MASK)
    assert m.pack_best(2, 5, 0) > m.pack_best(2, 6, m.TOK_MASK)


COUNTS_AT_THE_BOUNDARY = [(1 << 20) - 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1]


def _monotone_in_count(pack):
    """A pair's key never falls when its count rises (same ts and token), and it stays above a
    rival seen ten times: what phase 2's atomicMax relies on."""
    keys = [pack(c, 1000, 5) for c in COUNTS_AT_THE_BOUNDARY]
    return all(a <= b for a, b in zip(keys, keys[1:])) and all(k > pack(10, 0, 7) for k in keys)


def test_best_key_is_monotone_in_count_across_2_to_the_20():
    assert _monotone_in_count(m.pack_best)
    # saturated keys: equal count fields, so the earlier latest ts wins
    assert m.pack_best(1 << 20, 10, 5) > m.pack_best((1 << 20) + 7, 11, 6)
    assert m.unpack_best(m.pack_best((1 << 20) + 1, 1000, 5)) == (m.COUNT_MAX, 1000, 5)


def test_unclamped_best_key_wraps_at_2_to_the_20():
    """The layout before the clamp fails the same assertion, at exactly 2^20: count << 44 leaves the
    64-bit word and the key falls below a rival's with count 10."""
    assert not _monotone_in_count(m.pack_best_unclamped)
    assert m.pack_best_unclamped((1 << 20) - 1, 1000, 5) > m.pack_best_unclamped(10, 0, 7)
    assert m.pack_best_unclamped(1 << 20, 1000, 5) < m.pack_best_unclamped(10, 0, 7)


def test_full_table_sets_the_bit_and_drops_records():
    model = m.StoreModel("one", 3, 8, 8)
    model.initialize([[i % 97 for i in range(64)]], random.Random(0))
    assert model.status == m.SD_NGRAM_FULL
    assert sum(1 for k in model.gram_keys if k) == 8
    assert model.n_valid == sum(model.pair_count) < 62


def test_bad_tokens_are_dropped_with_the_bit():
    model = m.StoreModel("multi", 3, 64, 64)
    model.initialize([[1, 2, -1, 3, 4, 5], [1, 2, 3, 1 << 17, 1, 2]], random.Random(0))
    assert model.status == m.SD_NGRAM_BAD_TOKEN
    grams, pairs, best = model.decoded()
    assert grams == {(2, (3, 4)), (2, (1, 2))}
    assert {k: v[0] for k, v in pairs.items()} == {((2, (3, 4)), 5): 1, ((2, (1, 2)), 3): 1}
