"""A plain-Python, bit-exact model of what the device n-gram store (csrc/ngram_store.hip) keeps in
its two hash tables, written from the layout comment there and from include/specdec.h:

    gram table: key  = 1<<63 | level<<51 | t0 | t1<<17 | t2<<34      (level = the gram's order)
                best = min(count, 2^20-1)<<44 | (2^27-1-ts)<<17 | token
    pair table: key  = 1<<63 | gram_slot<<17 | token ; count u32 ; latest ts u32
    start slot = splitmix64(key) & (capacity-1), linear probing, 0 = empty

A call's records are applied as the kernels apply them: phase 1 (insert, count += 1, ts = max) over
ALL records in some order, then phase 2 (raise the gram's packed best key) over all records.  Slot
numbers depend on the insertion order, so what the model is compared by is the decoded content
(``decoded``): the set of grams, (gram, token) -> (count, ts), and gram -> best token.

``decode_tables`` decodes tables read back from a device store into the same three maps, and
``chain_stats`` measures the probe chains of a table (for the tests that need real collisions).
"""
from __future__ import annotations

import random
from typing import Dict, List, Optional, Sequence, Tuple

MASK64 = (1 << 64) - 1
USED = 1 << 63
TOK_BITS = 17
TOK_MASK = (1 << TOK_BITS) - 1
LEVEL_SHIFT = 51
TS_MAX = (1 << 27) - 1          # the record clock: ts in [0, 2^27-1)
TS_SHIFT = TOK_BITS
COUNT_SHIFT = 44
COUNT_MAX = (1 << 20) - 1       # the count field of the best key saturates here

SD_NGRAM_FULL = 1
SD_NGRAM_BAD_TOKEN = 2
SD_NGRAM_SATURATED = 4

Gram = Tuple[int, Tuple[int, ...]]   # (level, token ids oldest first)


def mix64(x: int) -> int:
    """splitmix64's finalizer."""
    x &= MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def gram_key(level: int, toks: Sequence[int]) -> int:
    assert 1 <= len(toks) <= 3 and all(0 <= t <= TOK_MASK for t in toks)
    k = USED | (level << LEVEL_SHIFT)
    for pos, t in enumerate(toks):
        k |= t << (TOK_BITS * pos)
    return k


def decode_gram_key(k: int) -> Gram:
    """(level, ids): the level says how many of the three id fields belong to the gram."""
    level = (k >> LEVEL_SHIFT) & 0xFFF
    return level, tuple((k >> (TOK_BITS * pos)) & TOK_MASK for pos in range(level))


def pair_key(gram_slot: int, token: int) -> int:
    assert 0 <= token <= TOK_MASK and gram_slot >= 0
    return USED | (gram_slot << TOK_BITS) | token


def decode_pair_key(k: int) -> Tuple[int, int]:
    return (k & ~USED & MASK64) >> TOK_BITS, k & TOK_MASK


def pack_best(count: int, ts: int, token: int) -> int:
    """The gram's best key: larger count wins, then the EARLIER latest ts.  The count field has 20
    bits and saturates at 2^20-1 (a count beyond it no longer raises the key)."""
    assert count >= 1 and 0 <= ts <= TS_MAX and 0 <= token <= TOK_MASK
    return (min(count, COUNT_MAX) << COUNT_SHIFT) | ((TS_MAX - ts) << TS_SHIFT) | token


def pack_best_unclamped(count: int, ts: int, token: int) -> int:
    """The layout before the clamp: count<<44 in 64 bits, which wraps to 0 at count = 2^20."""
    return ((count << COUNT_SHIFT) & MASK64) | ((TS_MAX - ts) << TS_SHIFT) | token


def unpack_best(b: int) -> Tuple[int, int, int]:
    """(count field, ts, token)"""
    return b >> COUNT_SHIFT, TS_MAX - ((b >> TS_SHIFT) & TS_MAX), b & TOK_MASK


def probe(keys: List[int], key: int, insert: bool) -> int:
    """Slot of key (inserted when absent if insert), -1 when absent or the table is full."""
    cap = len(keys)
    s = mix64(key) & (cap - 1)
    for _ in range(cap):
        if keys[s] == key:
            return s
        if keys[s] == 0:
            if not insert:
                return -1
            keys[s] = key
            return s
        s = (s + 1) & (cap - 1)
    return -1


class Record:
    __slots__ = ("gram", "level", "token", "ts")

    def __init__(self, level: int, gram: Sequence[int], token: int, ts: int):
        self.level, self.gram, self.token, self.ts = level, tuple(gram), token, ts

    def bad(self) -> bool:
        return any(t < 0 or t > TOK_MASK for t in self.gram + (self.token,))


class StoreModel:
    def __init__(self, kind: str, n: int, gram_capacity: int, pair_capacity: int):
        assert kind in ("one", "multi") and 2 <= n <= 4
        for c in (gram_capacity, pair_capacity):
            assert c > 0 and c & (c - 1) == 0
        self.kind, self.n = kind, n
        self.gram_keys = [0] * gram_capacity
        self.gram_best = [0] * gram_capacity
        self.pair_keys = [0] * pair_capacity
        self.pair_count = [0] * pair_capacity
        self.pair_ts = [0] * pair_capacity
        self.status = 0
        self.ts = 0            # the host's record clock
        self.n_valid = 0       # records applied (not skipped, not bad, not dropped by a full table)

    # ------------------------------------------------------------ a call's records
    def _levels(self) -> List[int]:
        return [self.n - 1] if self.kind == "one" else list(range(2, self.n))

    def initialize_records(self, rows: Sequence[Sequence[int]], ts_base: int) -> List[Record]:
        """Position i of row b records rows[b][i] after each gram of order j <= i ending there,
        stamped ts_base + b * len + i."""
        L = len(rows[0])
        out = []
        for b, row in enumerate(rows):
            assert len(row) == L
            for i in range(L):
                for j in self._levels():
                    if i >= j:
                        out.append(Record(j, row[i - j:i], row[i], ts_base + b * L + i))
        return out

    def update_records(self, rows: Sequence[Sequence[int]], nexts: Sequence[Sequence[int]],
                       ts_base: int) -> List[Record]:
        """next token k of row b after each gram ending the history, stamped ts_base + b * K + k
        (one level: only histories of at least n tokens; all orders: j <= len)."""
        L, K = len(rows[0]), len(nexts[0])
        out = []
        for b, (row, nxt) in enumerate(zip(rows, nexts)):
            assert len(row) == L and len(nxt) == K
            for j in self._levels():
                if (L >= self.n) if self.kind == "one" else (j <= L):
                    for k in range(K):
                        out.append(Record(j, row[L - j:], nxt[k], ts_base + b * K + k))
        return out

    def apply(self, records: List[Record], rng: Optional[random.Random] = None):
        """Phase 1 over every record in a permuted order, then phase 2 over every record."""
        order = list(range(len(records)))
        if rng is not None:
            rng.shuffle(order)
        slots: Dict[int, Tuple[int, int]] = {}
        for r in order:
            R = records[r]
            if R.bad():
                self.status |= SD_NGRAM_BAD_TOKEN
                continue
            gs = probe(self.gram_keys, gram_key(R.level, R.gram), True)
            ps = probe(self.pair_keys, pair_key(gs, R.token), True) if gs >= 0 else -1
            if ps < 0:
                self.status |= SD_NGRAM_FULL
                continue
            self.pair_count[ps] += 1
            self.pair_ts[ps] = max(self.pair_ts[ps], R.ts)
            self.n_valid += 1
            slots[r] = (gs, ps)
        if rng is not None:
            rng.shuffle(order)
        for r in order:
            if r not in slots:
                continue
            gs, ps = slots[r]
            if self.pair_count[ps] >= COUNT_MAX:
                self.status |= SD_NGRAM_SATURATED
            key = pack_best(self.pair_count[ps], self.pair_ts[ps], records[r].token)
            self.gram_best[gs] = max(self.gram_best[gs], key)

    def initialize(self, rows, rng: Optional[random.Random] = None):
        self.apply(self.initialize_records(rows, self.ts), rng)
        self.ts += len(rows) * len(rows[0])

    def update(self, rows, nexts, rng: Optional[random.Random] = None):
        self.apply(self.update_records(rows, nexts, self.ts), rng)
        self.ts += len(rows) * len(nexts[0])

    # ------------------------------------------------------------ what is observable
    def decoded(self):
        return decode_tables(self.gram_keys, self.gram_best, self.pair_keys, self.pair_count, self.pair_ts)


def decode_tables(gram_keys, gram_best, pair_keys, pair_count, pair_ts):
    """(grams, pairs, best): the set of (level, ids); (gram, token) -> (count, ts); gram -> token
    of its best key (grams whose best key is still 0 are left out of best)."""
    grams = {}
    for s, k in enumerate(gram_keys):
        if k:
            assert k & USED, hex(k)
            grams[s] = decode_gram_key(k)
    pairs = {}
    for s, k in enumerate(pair_keys):
        if k:
            assert k & USED, hex(k)
            gs, tok = decode_pair_key(k)
            assert gs in grams, (s, gs)      # a pair names an occupied gram slot
            assert (grams[gs], tok) not in pairs
            pairs[(grams[gs], tok)] = (pair_count[s], pair_ts[s])
    best = {grams[s]: gram_best[s] & TOK_MASK for s in grams if gram_best[s]}
    return set(grams.values()), pairs, best


def oracle_maps(store):
    """The same three maps from an oracle.specdec_ref.NgramStore (no ts: the oracle keeps none)."""
    grams = {(j, g) for j, per in store.counts.items() for g in per}
    counts = {((j, g), t): c for j, per in store.counts.items() for g, toks in per.items() for t, c in toks.items()}
    best = {(j, g): t for j, per in store.best.items() for g, t in per.items()}
    return grams, counts, best


def chain_stats(keys) -> Tuple[int, int, bool]:
    """(occupied slots, longest probe chain, whether a chain wraps from the last slot to slot 0) of
    a table, and a check that every key is reachable: probing from its start slot meets no empty
    slot before it."""
    cap = len(keys)
    used = longest = 0
    wraps = False
    for s, k in enumerate(keys):
        if not k:
            continue
        used += 1
        start = mix64(k) & (cap - 1)
        dist = (s - start) & (cap - 1)
        for d in range(dist):
            assert keys[(start + d) & (cap - 1)] != 0, ("unreachable key", hex(k), s, start)
        longest = max(longest, dist + 1)
        wraps |= start + dist >= cap
    return used, longest, wraps
