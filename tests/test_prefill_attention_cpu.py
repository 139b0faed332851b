"""CPU checks of sd_prefill_attention's host side: the ctypes mirror of its argument struct has the C layout, and
every shape, dtype or alignment the entry does not take is refused with SD_ERR_INVALID / SD_ERR_UNSUPPORTED before
anything is launched (fake device pointers, a null stream: a launch would not return these codes)."""
import ctypes as C

import pytest

from test_tree_attention_fp8_cpu import test_ctypes_layout_matches_the_header as _probe_layout

FAKE = 0x7f0000001000                                         # 16-byte aligned, never dereferenced by the host


def test_ctypes_layout_matches_the_header():
    _probe_layout("sd_prefill_attention_args")


def _args(paged=False, fp8=False):
    """A call the entry takes: B = 2, Hq = 8, Hkv = 2, R = 300, D = 128 over 512 positions (paged: 32 pages of 16)."""
    from specdec_amd import _lib
    a = _lib.sd_prefill_attention_args()
    a.batch, a.heads_q, a.heads_kv, a.rows, a.head_dim, a.dtype = 2, 8, 2, 300, 128, _lib.SD_BF16
    a.kv_cap, a.kv_alloc, a.kv_fp8, a.scale = 512, 512, int(fp8), 0.088
    a.q, a.k, a.v, a.out = FAKE, FAKE, FAKE, FAKE
    a.q_stride_b, a.q_stride_h, a.q_stride_r = 8 * 300 * 128, 300 * 128, 128
    a.k_stride_b, a.k_stride_h, a.k_stride_pos = a.v_stride_b, a.v_stride_h, a.v_stride_pos = 2 * 512 * 128, 512 * 128, 128
    a.out_stride_b, a.out_stride_r, a.out_stride_h = 300 * 8 * 128, 8 * 128, 128
    a.rows_add, a.kv_len_dev = 300, FAKE
    if fp8:
        a.k_scale = a.v_scale = FAKE
    if paged:
        a.block_table, a.block_table_stride_b, a.page_size, a.num_pages, a.max_pages = FAKE, 32, 16, 64, 32
        a.k_stride_page = a.v_stride_page = 2 * 16 * 128
        a.k_stride_h = a.v_stride_h = 16 * 128
    return a


BAD = [  # (what, paged, fp8, field values, accepted codes)
    ("null q", False, False, dict(q=None), "I"),
    ("null out", True, True, dict(out=None), "I"),
    ("fp32", False, False, dict(dtype="SD_F32"), "U"),
    ("D = 96", False, False, dict(head_dim=96), "U"),
    ("group 16", False, False, dict(heads_q=32), "U"),
    ("heads not divisible", False, False, dict(heads_q=7), "I"),
    ("rows 0", False, False, dict(rows=0), "IU"),
    ("rows 65537", False, False, dict(rows=65537), "U"),
    ("kv_cap above the limit", False, False, dict(kv_cap=(1 << 20) + 1, kv_alloc=(1 << 20) + 1), "U"),
    ("kv_cap > kv_alloc", False, False, dict(kv_cap=513), "I"),
    ("kv_cap > max_pages * S", True, False, dict(kv_cap=513), "I"),
    ("page size 48", True, False, dict(page_size=48), "IU"),
    ("FP8 without scales", False, True, dict(v_scale=None), "I"),
    ("FP8 stride of 8", True, True, dict(k_stride_pos=136), "I"),
    ("misaligned stride", False, False, dict(q_stride_r=132), "I"),
    ("misaligned pointer", False, False, dict(k=FAKE + 8), "I"),
    ("misaligned kv_len_dev", False, False, dict(kv_len_dev=FAKE + 4), "I"),
]


@pytest.mark.parametrize("what, paged, fp8, fields, codes", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_what_the_entry_does_not_take_is_refused_before_any_launch(what, paged, fp8, fields, codes):
    from specdec_amd import _lib
    a = _args(paged, fp8)
    for name, value in fields.items():
        setattr(a, name, getattr(_lib, value) if isinstance(value, str) else value)
    want = {"I": _lib.SD_ERR_INVALID, "U": _lib.SD_ERR_UNSUPPORTED}
    assert _lib.lib.sd_prefill_attention(C.byref(a), None) in [want[c] for c in codes], what


def test_null_args_are_invalid():
    from specdec_amd import _lib
    assert _lib.lib.sd_prefill_attention(None, None) == _lib.SD_ERR_INVALID
