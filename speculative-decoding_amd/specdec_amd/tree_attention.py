"""Tree attention inside a transformers model: the cached tree forwards without a mask tensor.

``"specdec_tree"`` is registered with transformers' ``AttentionInterface`` (and ``AttentionMaskInterface``).
A forward run under ``descriptors(model, ...)`` takes every layer's attention through
``ops.tree_attention`` (sd_tree_attention, the MFMA kernels of csrc/tree_attention.hip): the mask is the
per-row ``(kv_limit, win_bits)`` on the device and the host integer ``win_base``, all query heads of a
GQA group read one K/V stream, and transformers builds no mask at all.  Outside ``descriptors`` the name
behaves as the stock ``"sdpa"`` attention with the stock mask, so switching a model to it is harmless.
``descriptors_ragged`` is the same for a batch of sequences of different lengths: per-sequence device
tensors for the window base and the valid length, read by sd_tree_attention_ragged when it runs.
``causal(model, kv_len, ...)`` takes the plain causal forwards (a prompt, or a chunk of one behind a cached
prefix; any number of rows) through ``ops.prefill_attention`` (sd_prefill_attention) instead.

    dsc = row_descriptors(tree, cur, start, nodes, col_of)          # host lists, no [R, width] tensor
    if supported(model, len(dsc.kv_limit)):
        with descriptors(model, dsc, kv_len, device):
            out = model(input_ids=..., position_ids=..., past_key_values=cache)

``counts`` records which path each layer's attention took ("kernel" / "stock"), as
``sd_last_verify_path`` does for the verifies.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _lib, ops

NAME = "specdec_tree"
counts = {"kernel": 0, "stock": 0}     # attention calls (one per layer and forward) by the path they took


@dataclass
class RowDescriptors:
    """The mask of a cached forward's R new rows: row r sees key j when ``j < kv_limit[r]`` or bit
    ``j - win_base`` of ``win_bits[r]`` is set.  Host values; ``descriptors`` ships them."""
    kv_limit: List[int]
    win_bits: List[int]
    win_base: int


@dataclass
class _Active:
    kv_limit: torch.Tensor      # int32 [1, R] on the device ([B, R] under descriptors_ragged)
    win_bits: torch.Tensor      # int64 [1, R]
    win_base: object            # int; int64 [B] on the device under descriptors_ragged
    kv_len: object
    kv_cap: Optional[int] = None   # descriptors_ragged: the host's bound on every length
    k_scale: Optional[torch.Tensor] = None   # fp32 [Hkv]: the dequantisation scales of an FP8 cache, used when
    v_scale: Optional[torch.Tensor] = None   # the `key` an attention call receives is float8_e4m3fn
    causal: bool = False           # under `causal`: no descriptors, the rows are the last ones of kv_len


_active: Optional[_Active] = None


def row_descriptors(tr, cur: int, start: int, nodes, col_of) -> RowDescriptors:
    """``sampling.tree_decoding._allowed`` as descriptors: the forward feeds the committed tokens
    [start, cur), which are causal, then `nodes`; a node sees the committed tokens, its ancestors and
    itself, node j lying at position cur + col_of[j] (< 64: a tree has at most 64 nodes)."""
    limit = [start + r + 1 for r in range(cur - start)] + [cur] * len(nodes)
    bits = [0] * (cur - start)
    for i in nodes:
        bits.append(sum(1 << col_of[j] for j in tr.path_to(i)))
    return RowDescriptors(limit, bits, cur)


def supported(model, rows: int, max_rows: int = _lib.SD_TREE_ATTN_MAX_ROWS) -> bool:
    """Whether a forward of `rows` new tokens through `model` can take the kernel: a transformers model
    (its attention goes through the interface) of a 16-bit dtype with head_dim 64 or 128, at most
    SD_TREE_ATTN_MAX_GROUP query heads per K/V head and at most SD_TREE_ATTN_MAX_ROWS rows (max_rows:
    SD_PREFILL_ATTN_MAX_ROWS asks the same of a forward under ``causal``)."""
    cfg = getattr(model, "config", None)
    heads = getattr(cfg, "num_attention_heads", None)
    if cfg is None or not heads or not hasattr(cfg, "_attn_implementation"):
        return False
    kv_heads = getattr(cfg, "num_key_value_heads", None) or heads
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // heads
    return (getattr(model, "dtype", None) in (torch.bfloat16, torch.float16) and head_dim in (64, 128)
            and heads % kv_heads == 0 and heads // kv_heads <= _lib.SD_TREE_ATTN_MAX_GROUP
            and 1 <= rows <= max_rows and register())


@contextmanager
def descriptors(model, dsc: RowDescriptors, kv_len: int, device, k_scale=None, v_scale=None):
    """Run the forwards inside on the kernel: `model`'s attention implementation is "specdec_tree" for
    the block and every attention call reads `dsc` (batch 1) over the first `kv_len` cache positions.
    k_scale, v_scale (fp32 [Hkv] on the device): the scales of an FP8 cache; a call whose key is
    float8_e4m3fn then runs sd_tree_attention_fp8."""
    global _active
    if not register():
        raise RuntimeError("specdec_amd.tree_attention needs a transformers with AttentionInterface")
    signed = [b - (1 << 64) if b >> 63 else b for b in dsc.win_bits]      # the words as int64
    cfg, before, outer = model.config, model.config._attn_implementation, _active
    _active = _Active(torch.tensor([dsc.kv_limit], dtype=torch.int32).to(device, non_blocking=True),
                      torch.tensor([signed], dtype=torch.int64).to(device, non_blocking=True), int(dsc.win_base), int(kv_len),
                      k_scale=k_scale, v_scale=v_scale)
    cfg._attn_implementation = NAME
    try:
        yield
    finally:
        cfg._attn_implementation = before
        _active = outer


@contextmanager
def descriptors_ragged(model, kv_limit: torch.Tensor, win_bits: torch.Tensor, win_base: torch.Tensor, kv_len: torch.Tensor,
                       kv_cap: int, k_scale=None, v_scale=None):
    """``descriptors`` for a ragged batch, with everything on the device: kv_limit int32 [B, R], win_bits
    int64 [B, R], win_base and kv_len int64 [B] (sequence b's window base and valid length, the R new rows
    counted), kv_cap the host's bound on every length.  Every attention call inside runs
    sd_tree_attention_ragged, which reads them when its kernels run: the tensors may be overwritten in
    place between the replays of a captured forward.  k_scale, v_scale: as for ``descriptors``."""
    global _active
    if not register():
        raise RuntimeError("specdec_amd.tree_attention needs a transformers with AttentionInterface")
    cfg, before, outer = model.config, model.config._attn_implementation, _active
    _active = _Active(kv_limit, win_bits, win_base, kv_len, int(kv_cap), k_scale, v_scale)
    cfg._attn_implementation = NAME
    try:
        yield
    finally:
        cfg._attn_implementation = before
        _active = outer


@contextmanager
def causal(model, kv_len: int, device, k_scale=None, v_scale=None):
    """Run the plain causal forwards inside on sd_prefill_attention (batch 1): `model`'s attention implementation
    is "specdec_tree" for the block, no mask is built, and the R rows of every attention call are the last R of
    the first `kv_len` cache positions — a prompt (kv_len = R) or a chunk behind a cached prefix.  Any R up to
    SD_PREFILL_ATTN_MAX_ROWS.  k_scale, v_scale: as for ``descriptors``."""
    global _active
    if not register():
        raise RuntimeError("specdec_amd.tree_attention needs a transformers with AttentionInterface")
    cfg, before, outer = model.config, model.config._attn_implementation, _active
    _active = _Active(None, None, 0, int(kv_len), k_scale=k_scale, v_scale=v_scale, causal=True)
    cfg._attn_implementation = NAME
    try:
        yield
    finally:
        cfg._attn_implementation = before
        _active = outer


def _attention(module, query, key, value, attention_mask, scaling=None, dropout=0.0, **kwargs):
    """The ``AttentionInterface`` entry.  With descriptors: the kernel, out [B, R, Hq, D].  Without: the
    stock sdpa attention with the mask it was given."""
    d = _active
    if d is None:
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        counts["stock"] += 1
        return ALL_ATTENTION_FUNCTIONS["sdpa"](module, query, key, value, attention_mask, scaling=scaling,
                                               dropout=dropout, **kwargs)
    if d.causal:
        if key.dtype == torch.float8_e4m3fn and (d.k_scale is None or d.v_scale is None):
            raise RuntimeError("specdec_tree: an FP8 key needs k_scale and v_scale")
        scales = dict(k_scale=d.k_scale, v_scale=d.v_scale) if key.dtype == torch.float8_e4m3fn else {}
        out = ops.prefill_attention(query, key, value, d.kv_len, scale=scaling, **scales)
    elif key.dtype == torch.float8_e4m3fn:
        if d.k_scale is None or d.v_scale is None:
            raise RuntimeError("specdec_tree: an FP8 key needs descriptors with k_scale and v_scale")
        if d.kv_cap is not None:
            out = torch.ops.specdec.tree_attention_ragged_fp8(query, key, value, d.kv_limit, d.win_bits, d.win_base,
                                                              d.kv_len, d.k_scale, d.v_scale, scaling,
                                                              min(d.kv_cap, key.shape[2]))
        else:
            out = ops.tree_attention(query, key, value, d.kv_limit, d.win_bits, d.win_base, scale=scaling,
                                     kv_len=d.kv_len, k_scale=d.k_scale, v_scale=d.v_scale)
    elif d.kv_cap is not None:
        out = torch.ops.specdec.tree_attention_ragged(query, key, value, d.kv_limit, d.win_bits, d.win_base, d.kv_len,
                                                      scaling, min(d.kv_cap, key.shape[2]))
    else:
        out = ops.tree_attention(query, key, value, d.kv_limit, d.win_bits, d.win_base, scale=scaling, kv_len=d.kv_len)
    counts["kernel"] += 1
    return out, None


def _mask(*args, **kwargs):
    """The ``AttentionMaskInterface`` entry: no mask under descriptors, else the stock sdpa mask."""
    if _active is not None:
        return None
    from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS
    return ALL_MASK_ATTENTION_FUNCTIONS["sdpa"](*args, **kwargs)


def register() -> bool:
    """Register "specdec_tree" with transformers (idempotent); False when transformers lacks the interfaces."""
    try:
        from transformers import AttentionInterface
        from transformers.masking_utils import AttentionMaskInterface
    except ImportError:
        return False
    AttentionInterface.register(NAME, _attention)
    AttentionMaskInterface.register(NAME, _mask)
    return True
