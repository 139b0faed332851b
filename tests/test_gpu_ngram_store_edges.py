"""The device n-gram store (csrc/ngram_store.hip) where it can go wrong: tables small enough that
probe chains are long and wrap from the last slot to slot 0, thousands of threads on a handful of
slots, ids up to 2^17-1, ids out of range, strided C-ABI arguments, a full table, the end of the
record clock and the 20-bit count field of the best key.

Every answer is an integer, so every comparison is exact.  The tables are read back and decoded
into the maps of tests/ngram_store_model.py (grams, (gram, token) -> (count, ts), gram -> best
token) and compared with the oracle's restatement of ngram_assisted/ngram_storage.py; where the
record stamps matter too, with the host model of the tables."""
import ctypes as C

import pytest
import torch

import ngram_store_model as m
from oracle import specdec_ref as ref
from specdec_amd import _lib
from specdec_amd.ngram_assisted import DeviceNGramStorage, DeviceOneLevelNGramStorage, NGramStorage

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONFIGS = [("one", 2), ("one", 3), ("one", 4), ("multi", 2), ("multi", 3), ("multi", 4)]


def _make(kind, n, V, gcap, pcap):
    return (DeviceOneLevelNGramStorage if kind == "one" else DeviceNGramStorage)(
        n, V, device=DEV, gram_capacity=gcap, pair_capacity=pcap)


def _oracle(kind, n, V):
    return ref.NgramStore(kind, n, V, ref.TorchNoise(None))


def read_tables(dev):
    """The five tables as lists of unsigned Python ints."""
    u64 = [int(v) & m.MASK64 for v in torch.stack([dev._gram_keys, dev._gram_best]).cpu().flatten().tolist()]
    g = dev._gram_keys.numel()
    pk = [int(v) & m.MASK64 for v in dev._pair_keys.cpu().tolist()]
    pc = [int(v) & 0xFFFFFFFF for v in dev._pair_count.cpu().tolist()]
    pt = [int(v) & 0xFFFFFFFF for v in dev._pair_ts.cpu().tolist()]
    return u64[:g], u64[g:], pk, pc, pt


def decode(dev):
    return m.decode_tables(*read_tables(dev))


def assert_keys_well_formed(dev):
    """Non-zero keys are pairwise distinct (no key sits in two slots), carry bit 63, and hold
    nothing outside their fields: a gram key's ids above its level are 0, a pair names a gram slot
    inside the gram table."""
    gk, gb, pk, pc, pt = read_tables(dev)
    for keys in (gk, pk):
        nz = [k for k in keys if k]
        assert len(set(nz)) == len(nz)
        assert all(k >> 63 for k in nz)
    for k in gk:
        if k:
            level, ids = m.decode_gram_key(k)
            assert 1 <= level <= 3 and m.gram_key(level, ids) == k, hex(k)
    for s, k in enumerate(pk):
        if k:
            gs, tok = m.decode_pair_key(k)
            assert gs < len(gk) and gk[gs] and pc[s] >= 1, (s, hex(k))
        else:
            assert pc[s] == 0 and pt[s] == 0
    for s, k in enumerate(gk):
        assert k or gb[s] == 0


def assert_tables(dev, oracle):
    """The device tables hold exactly what the oracle recorded.  Returns the probe-chain figures
    of the two tables: (used, longest chain, wraps) each."""
    assert_keys_well_formed(dev)
    gk, gb, pk, pc, pt = read_tables(dev)
    grams, pairs, best = m.decode_tables(gk, gb, pk, pc, pt)
    want_grams, want_counts, want_best = m.oracle_maps(oracle)
    assert all(len(ids) == level for level, ids in grams)
    assert grams == want_grams                                    # level = the oracle's order
    assert {k: v[0] for k, v in pairs.items()} == want_counts
    assert sum(pc) == sum(want_counts.values())                   # one count per valid record
    assert best == want_best
    return m.chain_stats(gk), m.chain_stats(pk)                   # asserts every key is reachable


def _next_all(dev, oracle, hist, seed):
    """next_token of every history, with the same default-generator draws on both sides."""
    torch.manual_seed(seed)
    tok, known = dev.next_token(hist)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    want = [oracle.next_token(h) for h in hist.tolist()]
    assert torch.equal(state, torch.get_rng_state())
    assert tok.cpu().tolist() == [w[0] for w in want]
    assert known.cpu().tolist() == [w[1] for w in want]


def _want_has_gram(oracle, q):
    """The reference's has_gram: the gram is the LAST j ids, the queried token included."""
    if oracle.kind == "one":
        per = oracle.counts.get(oracle.n - 1, {}).get(tuple(q[-(oracle.n - 1):]), {})
        return len(q) >= oracle.n and q[-1] in per
    return any(q[-1] in oracle.counts.get(j, {}).get(tuple(q[-j:]), {}) for j in oracle._orders(len(q)))


def _pow2_at_least(x):
    c = 1
    while c < x:
        c *= 2
    return c


# ---------------------------------------------------------------------------------------------
# dense tables
# ---------------------------------------------------------------------------------------------
# (kind, n, symbols, first id, load target).  The alphabet size sets the number of distinct grams and
# pairs, hence the loads; the first id moves the hashes (the data seed of these cases: with every
# gram of the alphabet present, another random history gives the same key set), chosen on the host
# so that a chain of the gram table wraps past the last slot, which does not depend on the order of
# insertion.  The test asserts the loads, the wrap and the chain length.  NGramStorage(2) records
# no order at all (its orders are 2..n-1): its tables stay empty, which is what that case checks.
DENSE = [("one", 2, 16, 25, 0.5), ("one", 3, 8, 20, 0.5), ("one", 4, 4, 0, 0.5),
         ("multi", 2, 6, 0, 0.5), ("multi", 3, 8, 20, 0.5), ("multi", 4, 6, 9, 0.5),
         ("one", 3, 11, 0, 0.9)]
DENSE_FIGURES = {}


def _dense_data(S, first, B=8, L=200, steps=20):
    """B histories over the S ids first .. first+S-1 and 20 updates with k = 1, 3, 1, 3, ..."""
    g = torch.Generator().manual_seed(1)
    ids = first + torch.randint(0, S, (B, L), generator=g)
    nexts = [first + torch.randint(0, S, (B, 3 if step % 2 else 1), generator=g) for step in range(steps)]
    return ids, nexts


def _dense_capacities(kind, n, S, first, target):
    """Distinct grams and pairs of the whole run, from the oracle alone; the smallest powers of
    two that keep the load at or under the target (0.9 case: the smallest that is not full)."""
    ids, nexts = _dense_data(S, first)
    o = _oracle(kind, n, S + first)
    for row in ids.tolist():
        o.initialize(row)
    hist = ids
    for nx in nexts:
        for row, t in zip(hist.tolist(), nx.tolist()):
            o.update(row, t)
        hist = torch.cat([hist, nx[:, :1]], 1)
    grams, counts, _ = m.oracle_maps(o)
    G, P = len(grams), len(counts)
    if target >= 0.9:
        return G, P, _pow2_at_least(G + 1), _pow2_at_least(P + 1)
    return G, P, _pow2_at_least(int(G / target + 0.999999)), _pow2_at_least(int(P / target + 0.999999))


@pytest.mark.parametrize("kind,n,S,first,target", DENSE)
def test_dense_tables(kind, n, S, first, target):
    G, P, gcap, pcap = _dense_capacities(kind, n, S, first, target)
    if (kind, n) == ("multi", 2):
        assert G == P == 0
    elif target >= 0.9:
        assert 0.9 <= G / gcap < 1 and 0.9 <= P / pcap < 1, (G, gcap, P, pcap)
    else:
        assert 0.25 < G / gcap <= 0.5 and 0.25 < P / pcap <= 0.5, (G, gcap, P, pcap)
    ids, nexts = _dense_data(S, first)
    dev, o = _make(kind, n, S + first, gcap, pcap), _oracle(kind, n, S + first)
    dev.initialize(ids.to(DEV))
    for row in ids.tolist():
        o.initialize(row)
    stats = assert_tables(dev, o)
    hist = ids
    _next_all(dev, o, hist, 99)
    for step, nx in enumerate(nexts):
        dev.update(hist.to(DEV), nx.to(DEV))
        for row, t in zip(hist.tolist(), nx.tolist()):
            o.update(row, t)
        hist = torch.cat([hist, nx[:, :1]], 1)
        _next_all(dev, o, hist, step)
        if step % 5 == 4:
            stats = assert_tables(dev, o)
    assert dev.status() == 0
    (gu, glong, gwrap), (pu, plong, pwrap) = stats
    assert (gu, pu) == (G, P)
    DENSE_FIGURES[(kind, n, target)] = fig = dict(gram_load=G / gcap, pair_load=P / pcap, gram_cap=gcap, pair_cap=pcap,
                                                  longest_chain=max(glong, plong), wraps=gwrap or pwrap)
    print("dense", kind, n, target, fig)
    if G:
        assert fig["wraps"] and fig["longest_chain"] >= 4, fig     # else: choose another first id


# ---------------------------------------------------------------------------------------------
# contention
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("one", 2), ("one", 3), ("multi", 4)])
def test_contention_on_a_handful_of_slots(kind, n):
    B, L, S = 64, 300, 3
    row = torch.randint(0, S, (L,), generator=torch.Generator().manual_seed(3))
    ids = row.repeat(B, 1)
    o = _oracle(kind, n, S)
    for _ in range(B):
        o.initialize(row.tolist())
    grams, counts, _ = m.oracle_maps(o)
    dev = _make(kind, n, S, _pow2_at_least(2 * len(grams)), _pow2_at_least(2 * len(counts)))
    dev.initialize(ids.to(DEV))
    assert_tables(dev, o)
    _, pairs, _ = decode(dev)
    assert pairs and all(c % B == 0 for c, _ in pairs.values())
    _next_all(dev, o, ids, 5)
    assert dev.status() == 0


# ---------------------------------------------------------------------------------------------
# batching is invisible
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", CONFIGS)
def test_batched_and_row_by_row_initialize_leave_the_same_tables(kind, n):
    B, L, S = 4, 60, 4
    ids = torch.randint(0, S, (B, L), generator=torch.Generator().manual_seed(n))
    o = _oracle(kind, n, S)
    for row in ids.tolist():
        o.initialize(row)
    a, b = _make(kind, n, S, 256, 512), _make(kind, n, S, 256, 512)
    a.initialize(ids)
    for r in range(B):
        b.initialize(ids[r:r + 1])
    assert_tables(a, o)
    assert_tables(b, o)
    assert decode(a) == decode(b)                       # ts included
    model = m.StoreModel(kind, n, 256, 512)
    model.initialize(ids.tolist())
    assert decode(a) == model.decoded()


@pytest.mark.parametrize("kind,n", CONFIGS)
@pytest.mark.parametrize("prefix", ["n", "n-1"])
def test_initialize_and_per_token_updates_leave_the_same_tables(kind, n, prefix):
    """One history: initialize(whole) against initialize(prefix) + update(history[:i], [history[i]])
    for every later i.  The stamps agree (ts = i both ways).  The reference itself differs between
    the two for OneLevelNGramStorage when the prefix is shorter than n: its update skips histories
    of fewer than n tokens (ngram_storage.py:109-110), initialize records position n-1.  There the
    device follows the reference in each and the tables differ by exactly that record."""
    L, S = 80, 4
    P = n if prefix == "n" else n - 1
    row = torch.randint(0, S, (L,), generator=torch.Generator().manual_seed(10 + n)).tolist()
    o_a, o_c = _oracle(kind, n, S), _oracle(kind, n, S)
    a, c = _make(kind, n, S, 256, 512), _make(kind, n, S, 256, 512)
    o_a.initialize(row)
    a.initialize(torch.tensor([row]))
    o_c.initialize(row[:P])
    c.initialize(torch.tensor([row[:P]]))
    for i in range(P, L):
        o_c.update(row[:i], [row[i]])
        c.update(torch.tensor([row[:i]]), torch.tensor([[row[i]]]))
    assert_tables(a, o_a)
    assert_tables(c, o_c)
    assert a._ts == c._ts == L
    if m.oracle_maps(o_a) == m.oracle_maps(o_c):
        assert decode(a) == decode(c)                   # ts included
    else:
        assert kind == "one" and prefix == "n-1"
        assert decode(a) != decode(c)
        first = ((n - 1, tuple(row[:n - 1])), row[n - 1])
        ca, cc = m.oracle_maps(o_a)[1], m.oracle_maps(o_c)[1]
        assert ca[first] - cc.get(first, 0) == 1 and sum(ca.values()) - sum(cc.values()) == 1
    assert (m.oracle_maps(o_a) == m.oracle_maps(o_c)) == (not (kind == "one" and prefix == "n-1"))


# ---------------------------------------------------------------------------------------------
# wide ids
# ---------------------------------------------------------------------------------------------
WIDE = [0, 1, 65535, 65536, 131070, 131071]


@pytest.mark.parametrize("kind,n", CONFIGS)
def test_wide_ids(kind, n):
    """Grams that differ only in their top bits, or only in which position holds the large id: a
    shift or mask error in a key merges them."""
    V, B, L = 1 << 17, 4, 150
    g = torch.Generator().manual_seed(20 + n)
    wide = torch.tensor(WIDE)
    ids = wide[torch.randint(0, 6, (B, L), generator=g)]
    dev, o = _make(kind, n, V, 1024, 4096), _oracle(kind, n, V)
    dev.initialize(ids)
    for row in ids.tolist():
        o.initialize(row)
    hist = ids
    for step in range(4):
        nx = wide[torch.randint(0, 6, (B, 2), generator=g)]
        dev.update(hist, nx)
        for row, t in zip(hist.tolist(), nx.tolist()):
            o.update(row, t)
        hist = torch.cat([hist, nx[:, :1]], 1)
    assert_tables(dev, o)
    # every gram of up to 3 wide ids as a history: next_token, then has_gram on a sample
    queries = [[a] for a in WIDE] + [[a, b] for a in WIDE for b in WIDE] + \
              [[a, b, c] for a in WIDE for b in WIDE for c in WIDE]
    for length in (1, 2, 3):
        _next_all(dev, o, torch.tensor([q for q in queries if len(q) == length]), length)
    for q in queries[::5] + [h[-4:] for h in hist.tolist()]:
        assert dev.has_gram(torch.tensor(q)) == _want_has_gram(o, q), q
    _assert_chain(dev, o, hist[:, :L], 6)
    assert dev.status() == 0


# ---------------------------------------------------------------------------------------------
# draft_chain
# ---------------------------------------------------------------------------------------------
def _oracle_chain(o, rows, gamma, stop_if_unknown=False):
    """gamma chained next_token calls on the growing histories, step by step over the rows (the
    order of the default generator's draws); with stop_if_unknown (one row) the loop's early exit
    (ngram_assisted.py:94-101)."""
    rows = [list(r) for r in rows]
    drafts, known = [[] for _ in rows], [[] for _ in rows]
    for _ in range(gamma):
        for b, r in enumerate(rows):
            tok, kn = o.next_token(r)
            r.append(tok)
            drafts[b].append(tok)
            known[b].append(kn)
        if stop_if_unknown and not all(k[-1] for k in known):
            break
    return drafts, known


def _assert_chain(dev, o, hist, gamma, seed=7):
    torch.manual_seed(seed)
    drafts, known = dev.draft_chain(hist, gamma)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    want_d, want_k = _oracle_chain(o, hist.tolist(), gamma)
    assert torch.equal(state, torch.get_rng_state())
    assert tuple(drafts.shape) == tuple(known.shape) == (hist.shape[0], gamma)
    assert drafts.cpu().tolist() == want_d
    assert known.cpu().tolist() == want_k
    return want_k


@pytest.mark.parametrize("kind,n", CONFIGS)
def test_draft_chain_equals_chained_next_token(kind, n):
    V, S = 12, 5
    g = torch.Generator().manual_seed(40 + n)
    train = torch.randint(0, S, (2, 60), generator=g)      # a sparse store: many grams unknown,
    dev, o = _make(kind, n, V, 256, 1024), _oracle(kind, n, V)   # so fallback draws enter the chain
    dev.initialize(train)
    for row in train.tolist():
        o.initialize(row)
    flags = []
    for B in (1, 5):
        long_hist = torch.randint(0, S, (B, 33), generator=g)
        for length in sorted({0, 1, max(n - 2, 0), n - 1, 33}):
            hist = long_hist[:, :length]
            for gamma in (0, 1, 4, 8):
                flags += _assert_chain(dev, o, hist, gamma, seed=100 * B + gamma)
                # and the device's own next_token, call by call
                torch.manual_seed(100 * B + gamma)
                grown = hist
                for _ in range(gamma):
                    tok, kn = dev.next_token(grown)
                    grown = torch.cat([grown, tok.cpu().view(B, 1)], 1)
                state = torch.get_rng_state()
                torch.manual_seed(100 * B + gamma)
                drafts, _ = dev.draft_chain(hist, gamma)
                assert torch.equal(state, torch.get_rng_state())
                assert drafts.cpu().tolist() == grown[:, length:].tolist()
    if (kind, n) != ("multi", 2):
        # known and unknown steps both occurred, and in some chain an unknown step's fallback token
        # was part of a gram that the next step found
        assert any(any(k) for k in flags) and not all(all(k) for k in flags)
        assert any(not a and b for k in flags for a, b in zip(k, k[1:]))
    # stop_if_unknown, one row: the generator advances by exactly the calls the reference makes
    for gamma in (1, 4, 8):
        for trial in range(6):
            hist = torch.randint(0, S, (1, 20), generator=g)
            torch.manual_seed(trial)
            drafts, known = dev.draft_chain(hist, gamma, stop_if_unknown=True)
            state = torch.get_rng_state()
            torch.manual_seed(trial)
            want_d, want_k = _oracle_chain(o, hist.tolist(), gamma, stop_if_unknown=True)
            assert torch.equal(state, torch.get_rng_state()), (gamma, trial)
            made = len(want_d[0])
            assert drafts[0, :made].cpu().tolist() == want_d[0] and known[0, :made].cpu().tolist() == want_k[0]
    assert dev.status() == 0


def test_draft_chain_raises_keyerror_where_the_reference_does():
    """NGramStorage(4) after a 3-token prompt has created order 2 only: a lookup on 3 or more
    tokens indexes order 3 and raises KeyError (ngram_storage.py:171); shorter histories answer."""
    prompt = torch.tensor([[1, 2, 3]])
    dev, host = _make("multi", 4, 10, 64, 64), NGramStorage(4, 10)
    dev.initialize(prompt)
    host.initialize(prompt)
    for length in (0, 1, 2):
        hist = prompt[:, :length]
        torch.manual_seed(0)
        a = dev.next_token(hist)
        torch.manual_seed(0)
        b = host.next_token(hist)
        assert a[0].cpu().tolist() == b[0].tolist() and a[1].cpu().tolist() == b[1].tolist()
        dev.draft_chain(hist, 3 - length)               # the last call is on 2 tokens
        with pytest.raises(KeyError):
            dev.draft_chain(hist, 4 - length)           # the last call is on 3 tokens
    for length in (3, 4):
        hist = torch.tensor([[1, 2, 3, 1][:length]])
        with pytest.raises(KeyError):
            host.next_token(hist)
        with pytest.raises(KeyError):
            dev.next_token(hist)
        with pytest.raises(KeyError):
            dev.draft_chain(hist, 1)
        dev.draft_chain(hist, 0)


# ---------------------------------------------------------------------------------------------
# the C ABI directly: bad tokens, strides, empty histories
# ---------------------------------------------------------------------------------------------
def _c_initialize(dev, ids, ts_base, stride=None):
    B, L = ids.shape
    return _lib.lib.sd_ngram_store_initialize(C.byref(dev._s), ids.data_ptr(), B, L, stride or ids.stride(0), ts_base, None)


def _c_update(dev, ids, nxt, ts_base):
    B, L = ids.shape
    return _lib.lib.sd_ngram_store_update(C.byref(dev._s), ids.data_ptr(), B, L, ids.stride(0), nxt.data_ptr(),
                                          nxt.shape[1], nxt.stride(0), ts_base, None)


def _c_next(dev, ids, out, known):
    B, L = ids.shape
    return _lib.lib.sd_ngram_store_next_token(C.byref(dev._s), ids.data_ptr(), B, L, ids.stride(0), out.data_ptr(),
                                              known.data_ptr(), None)


def _c_draft(dev, ids, gamma, fb, drafts, known):
    B, L = ids.shape
    return _lib.lib.sd_ngram_store_draft(C.byref(dev._s), ids.data_ptr(), B, L, ids.stride(0), gamma, fb.data_ptr(),
                                         fb.stride(0), drafts.data_ptr(), drafts.stride(0), known.data_ptr(), None)


def _oracle_of_records(kind, n, V, records):
    """The oracle fed the clean records only, in the order of their stamps."""
    o = _oracle(kind, n, V)
    for R in sorted(records, key=lambda R: R.ts):
        if not R.bad():
            o._add(R.level, R.gram, [R.token])
    return o


@pytest.mark.parametrize("kind,n", [("one", 2), ("one", 3), ("multi", 3), ("multi", 4)])
def test_bad_tokens_are_dropped_and_reported(kind, n):
    V, B, L, S = 1 << 17, 5, 40, 4
    g = torch.Generator().manual_seed(60 + n)
    ids = torch.randint(0, S, (B, L), generator=g)
    ids[1, 17] = -1                       # inside row 1's history
    ids[3, 23] = 1 << 17                  # one past the largest id
    upd = torch.randint(0, S, (B, L), generator=g)
    upd[1, L - 1] = -1                    # the newest id of row 1: every gram of its update is bad
    nxt = torch.randint(0, S, (B, 3), generator=g)
    nxt[3, 1] = 1 << 17                   # a bad next token between two clean ones
    dev = _make(kind, n, V, 256, 512)
    model = m.StoreModel(kind, n, 256, 512)
    recs = model.initialize_records(ids.tolist(), 0) + model.update_records(upd.tolist(), nxt.tolist(), B * L)
    assert sum(R.bad() for R in recs) >= 6 and sum(not R.bad() for R in recs) > 100
    assert _c_initialize(dev, ids.to(DEV), 0) == _lib.SD_OK
    assert _c_update(dev, upd.to(DEV), nxt.to(DEV), B * L) == _lib.SD_OK
    assert dev.status() == _lib.SD_NGRAM_BAD_TOKEN
    o = _oracle_of_records(kind, n, V, recs)
    assert_tables(dev, o)                 # the clean rows' records, and those only
    grams, pairs, _ = decode(dev)
    assert all(0 <= t < S for _, toks in grams for t in toks) and all(0 <= t < S for _, t in pairs)
    model.initialize(ids.tolist())
    model.update(upd.tolist(), nxt.tolist())
    assert model.status == m.SD_NGRAM_BAD_TOKEN and decode(dev) == model.decoded()
    # lookups on histories whose newest id is out of range: unknown, the fallback left in place
    q = torch.randint(0, S, (4, 6), generator=g)
    q[0, -1], q[1, -1], q[2, -1] = -1, 1 << 17, -(1 << 40)
    qd = q.to(DEV)
    out = torch.tensor([101, 102, 103, 104], device=DEV)
    known = torch.full((4,), 7, dtype=torch.uint8, device=DEV)
    assert _c_next(dev, qd, out, known) == _lib.SD_OK
    assert out[:3].cpu().tolist() == [101, 102, 103] and known[:3].cpu().tolist() == [0, 0, 0]
    want_tok, want_known = o.next_token(q[3].tolist())           # the clean row beside them
    assert (int(out[3]), int(known[3])) == ((want_tok, 1) if want_known else (104, 0))
    fb = torch.tensor([[201, 202], [203, 204], [205, 206], [207, 208]], device=DEV) % S + 8
    drafts = torch.full((4, 2), -5, device=DEV)
    dknown = torch.full((4, 2), 7, dtype=torch.uint8, device=DEV)
    assert _c_draft(dev, qd, 2, fb, drafts, dknown) == _lib.SD_OK
    assert drafts[:3, 0].cpu().tolist() == fb[:3, 0].cpu().tolist() and dknown[:3, 0].cpu().tolist() == [0, 0, 0]
    assert dev.has_gram(q[0]) is False and dev.has_gram(q[1]) is False
    assert dev.status() == _lib.SD_NGRAM_BAD_TOKEN
    assert decode(dev) == model.decoded()                # lookups record nothing


POISON = (1 << 17) + 5


def _in_poison(t, width, lead=3):
    """t as a column slice of a wider buffer filled with an out-of-range id: the row stride
    exceeds the row length, and any read outside a row meets the poison."""
    wide = torch.full((t.shape[0] + 2, width), POISON, dtype=t.dtype, device=DEV)
    view = wide[1:-1, lead:lead + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) == width > t.shape[1] and not view.is_contiguous()
    return wide, view


@pytest.mark.parametrize("kind,n", [("one", 3), ("multi", 4)])
def test_strided_arguments_equal_contiguous_ones(kind, n):
    V, B, L, S, G = 1 << 17, 6, 50, 4, 5
    g = torch.Generator().manual_seed(70 + n)
    ids = torch.randint(0, S, (B, L), generator=g)
    nxt = torch.randint(0, S, (B, 3), generator=g)
    fb = torch.randint(0, V, (B, G), generator=g)
    a, b = _make(kind, n, V, 256, 512), _make(kind, n, V, 256, 512)
    _, ids_v = _in_poison(ids, L + 11)
    _, nxt_v = _in_poison(nxt, 9)
    _, fb_v = _in_poison(fb, G + 4)
    ids_c, nxt_c, fb_c = ids.to(DEV), nxt.to(DEV), fb.to(DEV)
    for dev, i, x in ((a, ids_c, nxt_c), (b, ids_v, nxt_v)):
        assert _c_initialize(dev, i, 0) == _lib.SD_OK
        assert _c_update(dev, i, x, B * L) == _lib.SD_OK
    assert a.status() == 0 and b.status() == 0           # no read met the poison
    assert decode(a) == decode(b)
    model = m.StoreModel(kind, n, 256, 512)
    model.initialize(ids.tolist())
    model.update(ids.tolist(), nxt.tolist())
    assert decode(b) == model.decoded()
    res = []
    for dev, i, f, strided in ((a, ids_c, fb_c, False), (b, ids_v, fb_v, True)):
        out = f[:, 0].clone()
        known = torch.zeros(B, dtype=torch.uint8, device=DEV)
        assert _c_next(dev, i, out, known) == _lib.SD_OK
        if strided:
            wide, drafts = _in_poison(torch.full((B, G), -1), G + 6, lead=2)
        else:
            wide, drafts = None, torch.full((B, G), -1, device=DEV)
        dknown = torch.zeros(B, G, dtype=torch.uint8, device=DEV)
        assert _c_draft(dev, i, G, f, drafts, dknown) == _lib.SD_OK
        res.append((out.cpu().tolist(), known.cpu().tolist(), drafts.cpu().tolist(), dknown.cpu().tolist()))
        if strided:
            mask = torch.ones_like(wide, dtype=torch.bool)
            mask[1:-1, 2:2 + G] = False
            assert bool((wide[mask] == POISON).all())    # the poison around drafts is untouched
            assert bool((drafts >= 0).all()) and bool((drafts < V).all())
    assert res[0] == res[1]
    assert any(res[0][1]) and any(any(r) for r in res[0][3])
    assert a.status() == 0 and b.status() == 0


@pytest.mark.parametrize("kind,n", [("one", 3), ("multi", 3)])
def test_empty_histories_launch_and_change_nothing(kind, n):
    """len = 0 with rows to answer: the kernels run, find no gram, record nothing."""
    dev = _make(kind, n, 50, 64, 64)
    dev.initialize(torch.tensor([[1, 2, 3, 1, 2, 3]]))
    before = read_tables(dev)
    empty = torch.zeros(3, 0, dtype=torch.long, device=DEV)
    nxt = torch.tensor([[4], [5], [6]], device=DEV)
    assert _c_update(dev, empty, nxt, dev._ts) == _lib.SD_OK
    out = torch.tensor([11, 12, 13], device=DEV)
    known = torch.full((3,), 7, dtype=torch.uint8, device=DEV)
    assert _c_next(dev, empty, out, known) == _lib.SD_OK
    assert out.cpu().tolist() == [11, 12, 13] and known.cpu().tolist() == [0, 0, 0]
    assert dev.has_gram(torch.zeros(0, dtype=torch.long)) is False
    assert read_tables(dev) == before and dev.status() == 0


# ---------------------------------------------------------------------------------------------
# a full table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("one", 3), ("multi", 4)])
def test_full_table_behaviour(kind, n):
    """The one test with a weaker-than-exact property: dropped records change counts, so what is
    stored is bounded by the oracle, not equal to it."""
    V = 100
    row = (torch.arange(64) % 97).repeat(3).view(1, -1)          # far more grams than 8 slots
    dev, o = _make(kind, n, V, 8, 8), _oracle(kind, n, V)
    dev.initialize(row)
    dev.update(row, torch.tensor([[5, 6, 7]]))
    torch.cuda.synchronize()                                     # the calls return
    o.initialize(row[0].tolist())
    o.update(row[0].tolist(), [5, 6, 7])
    assert dev.status() == _lib.SD_NGRAM_FULL
    assert_keys_well_formed(dev)
    gk, gb, pk, pc, pt = read_tables(dev)
    assert all(gk)                                               # the gram table is full
    grams, pairs, best = m.decode_tables(gk, gb, pk, pc, pt)
    _, want_counts, _ = m.oracle_maps(o)
    for (gram, tok), (count, _) in pairs.items():
        assert 1 <= count <= want_counts[(gram, tok)]            # KeyError: a pair nobody recorded
    for gram, tok in best.items():
        assert (gram, tok) in want_counts and (gram, tok) in pairs
    # lookups: a present gram answers with a token the oracle recorded after it (all orders: after
    # it or, when its own slot holds no best yet, after a shorter suffix of it)
    for level, ids in sorted(grams):
        tok, known = dev.next_token(torch.tensor([list(ids)]))
        if (level, ids) in best:
            assert bool(known[0])
        if bool(known[0]):
            assert any(((j, ids[-j:]), int(tok[0])) in want_counts for j in range(1, level + 1))
    # an absent gram: the probe visits every slot of the full table once and reports unknown
    for level in {lv for lv, _ in grams}:
        tok, known = dev.next_token(torch.tensor([[90 + i for i in range(level)]]))
        assert not bool(known[0])
    assert dev.has_gram(torch.tensor([91, 92, 93, 94])) is False
    dev.reset()
    assert dev.status() == 0 and dev._ts == 0
    small = torch.tensor([[1, 2, 3, 1, 2, 3, 1, 2, 4]])
    o2 = _oracle(kind, n, V)
    dev.initialize(small)
    o2.initialize(small[0].tolist())
    assert_tables(dev, o2)
    assert dev.status() == 0


# ---------------------------------------------------------------------------------------------
# the record clock
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("one", 2), ("multi", 3)])
def test_record_clock_runs_to_its_end_and_stops(kind, n):
    """The last 2^27-1 - N stamps: a tie-heavy history of exactly N records takes the key's ts field
    to its smallest value; the call that would pass the limit is refused and changes nothing."""
    S, B, L = 3, 2, 30
    g = torch.Generator().manual_seed(80 + n)
    ids = torch.randint(0, S, (B, L), generator=g)
    nexts = [torch.randint(0, S, (B, k), generator=g) for k in (1, 3, 1, 3, 2)]
    N = B * L + sum(B * nx.shape[1] for nx in nexts)
    dev, o = _make(kind, n, S, 64, 128), _oracle(kind, n, S)
    model = m.StoreModel(kind, n, 64, 128)
    dev._ts = model.ts = m.TS_MAX - N
    dev.initialize(ids)
    model.initialize(ids.tolist())
    for row in ids.tolist():
        o.initialize(row)
    hist = ids
    for nx in nexts:
        dev.update(hist, nx)
        model.update(hist.tolist(), nx.tolist())
        for row, t in zip(hist.tolist(), nx.tolist()):
            o.update(row, t)
        hist = torch.cat([hist, nx[:, :1]], 1)
    assert dev._ts == m.TS_MAX
    assert_tables(dev, o)
    assert decode(dev) == model.decoded()
    _, pairs, _ = decode(dev)
    assert max(ts for _, ts in pairs.values()) == m.TS_MAX - 1   # the newest stamp there is
    assert min(m.unpack_best(b)[1] for b in read_tables(dev)[1] if b) >= m.TS_MAX - N
    _next_all(dev, o, hist, 1)
    before = read_tables(dev)
    with pytest.raises(_lib.SpecdecError, match="-4"):
        dev.update(hist, nexts[0])
    with pytest.raises(_lib.SpecdecError, match="-4"):
        dev.initialize(ids[:1, :1])
    assert _c_update(dev, hist.to(DEV), nexts[0].to(DEV), dev._ts) == _lib.SD_ERR_UNSUPPORTED
    assert dev._ts == m.TS_MAX and read_tables(dev) == before and dev.status() == 0


# ---------------------------------------------------------------------------------------------
# the count field at 2^20
# ---------------------------------------------------------------------------------------------
def _saturating_row():
    """(5)->5 recorded 2^20 + 3 times, (5)->7 ten times, (7)->5 ten times, (7)->7 once."""
    head = [5, 5, 5, 7] * 9 + [5, 5, 5, 7, 7]
    run = (1 << 20) + 3 - 20 + 1
    row = torch.full((len(head) + run,), 5, dtype=torch.long)
    row[:len(head)] = torch.tensor(head)
    return row.view(1, -1)


def _assert_saturated_answers(dev):
    tok, known = dev.next_token(torch.tensor([[5]]))
    assert bool(known[0])
    assert int(tok[0]) == 5          # before the clamp: 7, the rival seen ten times
    # the reference's has_gram looks up the LAST n-1 ids, the queried token included: (7) -> 7
    assert dev.has_gram(torch.tensor([5, 7])) is True
    assert dev.has_gram(torch.tensor([7, 5])) is True      # (5) -> 5
    assert dev.has_gram(torch.tensor([5, 9])) is False
    _, pairs, best = decode(dev)
    assert {k: v[0] for k, v in pairs.items()} == {((1, (5,)), 5): (1 << 20) + 3, ((1, (5,)), 7): 10,
                                                   ((1, (7,)), 5): 10, ((1, (7,)), 7): 1}
    assert best == {(1, (5,)): 5, (1, (7,)): 5}


def test_count_field_saturates_at_2_to_the_20():
    """One initialize raises (5)->5 from nothing past 2^20: every key phase 2 offers for it carries
    the final count.  Unclamped, (2^20 + 3) << 44 wraps to 3 << 44 and the rival with count 10 wins."""
    dev = _make("one", 2, 16, 16, 16)
    row = _saturating_row()
    assert row.numel() * 8 < 9 << 20
    dev.initialize(row)
    _assert_saturated_answers(dev)
    assert dev.status() == _lib.SD_NGRAM_SATURATED
    assert m.unpack_best(read_tables(dev)[1][m.probe(read_tables(dev)[0], m.gram_key(1, (5,)), False)])[0] == m.COUNT_MAX


def test_count_field_split_over_two_calls_keeps_its_stale_key():
    """The same row in two calls at its midpoint: the first call's key (count about 2^19) stays in
    gram_best and outranks the rival whatever the second call offers: keys only grow."""
    dev = _make("one", 2, 16, 16, 16)
    row = _saturating_row()
    mid = row.numel() // 2
    dev.initialize(row[:, :mid])
    # the second call repeats the boundary token so that no 5 -> 5 transition is lost
    dev.initialize(row[:, mid - 1:])
    _assert_saturated_answers(dev)
    assert dev.status() & ~_lib.SD_NGRAM_SATURATED == 0
