"""KV-cache prune (utils/caching.py:6-77).

The prune is metadata-only: drop the last k positions of every K/V tensor.  A transformers-5
StaticCache is cropped ON THE DEVICE by the verify kernel's prune output (prune_static_cache).  The verify kernel
returns k per sequence (prune_drafter = γ'-n, prune_target = γ'-n+1,
sampling/speculative_decoding.py:163-165).  Unlike the reference, the DynamicCache branch works
on transformers 5.x (the reference reads the removed ``key_cache``/``_seen_tokens``):
it calls ``DynamicCache.crop(-k)``, the transformers-5 way to drop the last k positions.

Reference semantics kept on purpose: the tuple path slices ``[:, :, :-k, :]`` (:51), so k = 0
returns EMPTY K/V views, exactly as the reference does (its loops never prune 0 positions:
the prune only runs after a reject, k_drafter >= 1, k_target >= 2).

``compact_cache`` is the tree loop's counterpart (sampling/tree_decoding.py; no reference code): a crop
is not enough after a tree verify, the accepted nodes lie scattered among rejected siblings, so one
sd_kv_compact launch moves them to the front of the tree's window in every layer before the length is
set.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

try:  # transformers is optional for the tuple path
    from transformers.cache_utils import DynamicCache
except Exception:  # pragma: no cover
    DynamicCache = None


def _static_lengths(cache):
    """The per-layer device length tensors of a transformers-5 StaticCache (StaticLayer keeps the
    cached length as a device tensor, ``cumulative_length``, and writes new keys at it), or None."""
    layers = getattr(cache, "layers", None)
    if not layers:
        return None
    lens = [getattr(layer, "cumulative_length", None) for layer in layers]
    if not all(torch.is_tensor(t) for t in lens):
        return None
    return lens


def prune_cache(cache, num_tokens_to_discard: Union[int, Tensor]):
    """utils/caching.py:6-24: tuple caches -> views, cache objects -> cropped in place.

    num_tokens_to_discard may be a device tensor (the verify kernel's ``prune_*`` output) for a
    StaticCache: the crop then runs on the device, driven by the kernel, with no host read."""
    if cache is None:
        return None
    if _static_lengths(cache) is not None:
        return prune_static_cache(cache, num_tokens_to_discard)
    if torch.is_tensor(num_tokens_to_discard):
        num_tokens_to_discard = int(num_tokens_to_discard.reshape(-1)[0].item())   # host crop: one read
    if isinstance(cache, tuple):
        return prune_tuple_cache(cache, num_tokens_to_discard)
    if (DynamicCache is not None and isinstance(cache, DynamicCache)) or hasattr(cache, "crop"):
        return prune_dynamic_cache(cache, num_tokens_to_discard)
    raise ValueError("Unsupported cache type.")


def prune_tuple_cache(cache: Tuple[Tuple[Tensor, Tensor]], num_tokens_to_discard: int):
    """utils/caching.py:27-55: views without the last k positions (dim 2) of every K/V tensor."""
    if cache is None:
        return None
    out = []
    for layer in cache:
        if layer is None:
            out.append(None)
            continue
        out.append(tuple(t[:, :, :-num_tokens_to_discard, :] for t in layer))
    return tuple(out)


def prune_dynamic_cache(cache, num_tokens_to_discard: int):
    """utils/caching.py:58-77, on the transformers-5 API: drop the last k positions of every layer
    in place (``crop(-k)``; the reference's ``key_cache`` / ``_seen_tokens`` no longer exist)."""
    if cache is None:
        return None
    if num_tokens_to_discard > 0:
        cache.crop(-int(num_tokens_to_discard))
    return cache


def prune_static_cache(cache, num_tokens_to_discard: Union[int, Tensor]):
    """Device-side crop of a transformers-5 StaticCache: the K/V buffers keep
    their addresses and the stale positions are overwritten by the next write (the causal mask
    built from ``cache_position`` hides them meanwhile), so dropping the last k positions is
    ``cumulative_length -= k`` in every layer — one multi-tensor launch.  k is an int, or a device
    tensor of one element (batch 1, as the reference's prune; ``prune_*[0]`` of a verify), which
    keeps the crop on the device without a host read.  k = 0 is a no-op, so a loop can apply the
    kernel's prune output every step without branching on it."""
    lens = _static_lengths(cache)
    if lens is None:
        raise ValueError("not a StaticCache")
    if torch.is_tensor(num_tokens_to_discard):
        k = num_tokens_to_discard.reshape(-1)[:1].reshape(())
        torch._foreach_sub_(lens, k.to(device=lens[0].device, dtype=lens[0].dtype))
    elif num_tokens_to_discard:
        torch._foreach_sub_(lens, int(num_tokens_to_discard))
    return cache



def _kv_groups(tensors):
    """The tensors grouped by (shape, strides, dtype): one sd_kv_compact call serves one layout (K and V
    of a model whose head sizes differ form two groups)."""
    groups = {}
    for t in tensors:
        groups.setdefault((tuple(t.shape), t.stride(), t.dtype), []).append(t)
    return list(groups.values())


def compact_cache(cache, path: Tensor, count: Tensor, base: int, *, num_slots: int, node_slot=None,
                  new_length: Optional[int] = None):
    """Compact a KV cache onto the accepted path of a token tree and set its length.

    The cache holds the tree's nodes at positions ``base + slot(i)`` (``slot(i) = node_slot[i]``, or i).
    ``path`` (int32 [B, depth]) and ``count`` (int32 [B]) are ``verify_tree``'s device outputs
    (``path``, ``n_accepted``): in every K/V tensor of every layer, position ``base + slot(path[b, d])``
    moves to ``base + d`` for d < count[b] — ONE kernel launch for the whole cache, nothing read back —
    and the cache's length becomes ``new_length`` (normally base + count).

    DynamicCache (transformers 5): ``layer.keys`` / ``layer.values`` compacted, then ``crop`` to
    new_length (a host int, required).  StaticCache: compacted, then ``cumulative_length`` of every
    layer set on the device in one multi-tensor call — ``new_length``, or ``base + count[0]`` computed
    on the device when it is None.  A tuple cache: compacted, the sliced views returned.  Anything
    else raises ValueError("Unsupported cache type.")."""
    from ..ops import kv_compact
    lens = _static_lengths(cache)
    if lens is not None:
        tensors = [t for layer in cache.layers for t in (layer.keys, layer.values)]
    elif isinstance(cache, tuple):
        tensors = [t for layer in cache if layer is not None for t in layer]
    elif DynamicCache is not None and isinstance(cache, DynamicCache):
        tensors = [t for layer in cache.layers for t in (layer.keys, layer.values)]
    else:
        raise ValueError("Unsupported cache type.")
    if lens is None and new_length is None:
        raise ValueError("compact_cache: new_length (a host int) is needed to crop this cache")
    for group in _kv_groups(tensors):
        kv_compact(group, path, count, base, num_slots=num_slots, node_slot=node_slot)
    if lens is not None:
        if new_length is None:
            length = (count.reshape(-1)[0] + int(base)).to(lens[0].dtype)
        else:
            length = torch.full((), int(new_length), dtype=lens[0].dtype, device=lens[0].device)
        torch._foreach_copy_(lens, [length] * len(lens))
        return cache
    new_length = int(new_length)
    if isinstance(cache, tuple):
        return tuple(None if layer is None else tuple(t[:, :, :new_length, :] for t in layer) for layer in cache)
    drop = tensors[0].shape[2] - new_length
    if drop > 0:
        cache.crop(-drop)                       # the negative form: remove `drop` positions
    return cache
