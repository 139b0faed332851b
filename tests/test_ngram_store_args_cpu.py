"""Argument checks of the five sd_ngram_store_* entry points (csrc/ngram_store.hip).  Every refusal
here, and every empty call, returns before a kernel is launched, so no device is needed: the table
and tensor pointers are host buffers that a correct library never reads or writes."""
import ctypes as C

import pytest

from specdec_amd import _lib

P = 0x1000          # a non-null address for pointers that must not be dereferenced
TABLE_FIELDS = ("gram_keys", "gram_best", "pair_keys", "pair_count", "pair_ts", "status")
POISON = 0x5A


class Buffers:
    """Host memory behind every pointer of a call, poisoned, to show that nothing was touched."""

    def __init__(self):
        self.bufs = {name: (C.c_uint8 * 256)(*([POISON] * 256))
                     for name in TABLE_FIELDS + ("ids", "next", "out", "known", "fallback", "drafts")}

    def ptr(self, name):
        return C.addressof(self.bufs[name])

    def untouched(self):
        return all(bytes(b) == bytes([POISON]) * 256 for b in self.bufs.values())

    def store(self, **over):
        f = dict(gram_keys=self.ptr("gram_keys"), gram_best=self.ptr("gram_best"), gram_capacity=16,
                 pair_keys=self.ptr("pair_keys"), pair_count=self.ptr("pair_count"), pair_ts=self.ptr("pair_ts"),
                 pair_capacity=32, status=self.ptr("status"), n=3, one_level=0, vocab=1 << 17)
        f.update(over)
        return _lib.sd_ngram_store(*[f[name] for name, _ in _lib.sd_ngram_store._fields_])


def _entries(bufs):
    """name -> (call(store pointer, **overrides), the arguments it has)"""
    lib = _lib.lib
    ids, nxt, out, known = bufs.ptr("ids"), bufs.ptr("next"), bufs.ptr("out"), bufs.ptr("known")
    fb, drafts = bufs.ptr("fallback"), bufs.ptr("drafts")

    def initialize(s, batch=2, len=4, ts_base=0, **_):
        return lib.sd_ngram_store_initialize(s, ids, batch, len, 4, ts_base, None)

    def update(s, batch=2, len=4, ts_base=0, k=2, **_):
        return lib.sd_ngram_store_update(s, ids, batch, len, 4, nxt, k, 2, ts_base, None)

    def next_token(s, batch=2, len=4, **_):
        return lib.sd_ngram_store_next_token(s, ids, batch, len, 4, out, known, None)

    def draft(s, batch=2, len=4, gamma=3, **_):
        return lib.sd_ngram_store_draft(s, ids, batch, len, 4, gamma, fb, 3, drafts, 3, known, None)

    def has_gram(s, len=4, **_):
        return lib.sd_ngram_store_has_gram(s, ids, len, out, None)

    return {"initialize": (initialize, {"batch", "len", "ts_base"}),
            "update": (update, {"batch", "len", "ts_base", "k"}),
            "next_token": (next_token, {"batch", "len"}),
            "draft": (draft, {"batch", "len", "gamma"}),
            "has_gram": (has_gram, {"len"})}


ENTRY_NAMES = ("initialize", "update", "next_token", "draft", "has_gram")


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_bad_stores_are_refused(entry):
    bufs = Buffers()
    call, _ = _entries(bufs)[entry]
    assert call(None) == _lib.SD_ERR_INVALID                                   # null store
    bad = [{f: None} for f in TABLE_FIELDS]                                     # a null table pointer
    bad += [{"gram_capacity": c} for c in (0, -16, 3, 24, (1 << 20) + 1)]       # not a power of two
    bad += [{"pair_capacity": c} for c in (0, -32, 3, 48, (1 << 21) - 1)]
    bad += [{"n": 1}, {"n": 5}, {"n": 0}, {"n": -3}]
    bad += [{"vocab": (1 << 17) + 1}, {"vocab": 0}, {"vocab": -1}]
    for over in bad:
        s = bufs.store(**over)
        assert call(C.byref(s)) == _lib.SD_ERR_INVALID, (entry, over)
    assert bufs.untouched()


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_bad_shapes_are_refused(entry):
    bufs = Buffers()
    call, has = _entries(bufs)[entry]
    s = bufs.store()
    bad = [{"batch": -1}, {"len": -1}, {"ts_base": -1}, {"k": 0}, {"k": -2}, {"gamma": -1}]
    tried = 0
    for over in bad:
        if set(over) <= has:
            assert call(C.byref(s), **over) == _lib.SD_ERR_INVALID, (entry, over)
            tried += 1
    assert tried >= 1 and bufs.untouched()


def test_null_tensors_are_refused():
    bufs = Buffers()
    lib, s = _lib.lib, bufs.store()
    sp, ids, nxt, out, known = C.byref(s), bufs.ptr("ids"), bufs.ptr("next"), bufs.ptr("out"), bufs.ptr("known")
    fb, dr = bufs.ptr("fallback"), bufs.ptr("drafts")
    inv = _lib.SD_ERR_INVALID
    assert lib.sd_ngram_store_initialize(sp, None, 2, 4, 4, 0, None) == inv
    assert lib.sd_ngram_store_update(sp, None, 2, 4, 4, nxt, 2, 2, 0, None) == inv
    assert lib.sd_ngram_store_update(sp, ids, 2, 4, 4, None, 2, 2, 0, None) == inv
    assert lib.sd_ngram_store_next_token(sp, None, 2, 4, 4, out, known, None) == inv
    assert lib.sd_ngram_store_next_token(sp, ids, 2, 4, 4, None, known, None) == inv
    assert lib.sd_ngram_store_next_token(sp, ids, 2, 4, 4, out, None, None) == inv
    assert lib.sd_ngram_store_draft(sp, None, 2, 4, 4, 3, fb, 3, dr, 3, known, None) == inv
    assert lib.sd_ngram_store_draft(sp, ids, 2, 4, 4, 3, None, 3, dr, 3, known, None) == inv
    assert lib.sd_ngram_store_draft(sp, ids, 2, 4, 4, 3, fb, 3, None, 3, known, None) == inv
    assert lib.sd_ngram_store_draft(sp, ids, 2, 4, 4, 3, fb, 3, dr, 3, None, None) == inv
    assert lib.sd_ngram_store_has_gram(sp, None, 4, out, None) == inv
    assert lib.sd_ngram_store_has_gram(sp, ids, 4, None, None) == inv
    assert bufs.untouched()


def test_empty_calls_return_ok_and_touch_nothing():
    """batch = 0 everywhere, len = 0 for initialize and gamma = 0 for draft: no record, no launch.
    (len = 0 with rows to answer launches a kernel: tests/test_gpu_ngram_store_edges.py.)"""
    bufs = Buffers()
    e = _entries(bufs)
    sp = C.byref(bufs.store())
    assert e["initialize"][0](sp, batch=0) == _lib.SD_OK
    assert e["initialize"][0](sp, len=0) == _lib.SD_OK
    assert e["initialize"][0](sp, batch=0, len=0) == _lib.SD_OK
    assert e["update"][0](sp, batch=0) == _lib.SD_OK
    assert e["update"][0](sp, batch=0, len=0) == _lib.SD_OK
    assert e["next_token"][0](sp, batch=0) == _lib.SD_OK
    assert e["next_token"][0](sp, batch=0, len=0) == _lib.SD_OK
    assert e["draft"][0](sp, batch=0) == _lib.SD_OK
    assert e["draft"][0](sp, gamma=0) == _lib.SD_OK
    assert e["draft"][0](sp, batch=0, len=0, gamma=0) == _lib.SD_OK
    assert bufs.untouched()


def test_the_record_clock_limit_is_checked_before_any_launch():
    """ts_base + the call's records may reach 2^27-1 and not pass it; an empty call at the limit is
    still an empty call."""
    bufs = Buffers()
    e = _entries(bufs)
    sp = C.byref(bufs.store())
    top = (1 << 27) - 1
    assert e["initialize"][0](sp, batch=2, len=4, ts_base=top - 7) == _lib.SD_ERR_UNSUPPORTED
    assert e["update"][0](sp, batch=2, k=2, ts_base=top - 3) == _lib.SD_ERR_UNSUPPORTED
    assert e["initialize"][0](sp, batch=0, ts_base=top) == _lib.SD_OK
    assert e["update"][0](sp, batch=0, ts_base=top) == _lib.SD_OK
    assert bufs.untouched()
