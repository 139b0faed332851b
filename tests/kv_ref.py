"""Host model of sd_kv_compact (include/specdec.h): the rule as a sequential loop in pure torch, on
whatever device the tensors live.  Tests run it on a clone and compare bit for bit."""
import torch

MAX_NODES, MAX_DEPTH = 64, 32          # SD_TREE_MAX_NODES, SD_MAX_GAMMA


def compact(tensors, path, count, base, num_slots, node_slot=None):
    """In place on `tensors` ([B, H, L, D] each): for every sequence b and depth d < min(count[b],
    path.shape[1], 32), IN ASCENDING d, row base + slot(path[b][d]) is copied to row base + d.  A path
    entry outside [0, 64) or a slot outside [d, num_slots) ends the sequence's moves.  Returns True when
    some sequence ended that way (the kernel ORs SD_ROW_INVALID_DIST into status_or then)."""
    path = torch.as_tensor(path).cpu().tolist()
    count = torch.as_tensor(count).cpu().tolist()
    flagged = False
    for b in range(len(count)):
        for d in range(min(count[b], len(path[b]), MAX_DEPTH)):
            p = path[b][d]
            s = -1
            if 0 <= p < MAX_NODES:
                s = p if node_slot is None else (node_slot[p] if p < len(node_slot) else -1)
            if not d <= s < num_slots:
                flagged = True
                break
            if s != d:
                for t in tensors:
                    t[b, :, base + d] = t[b, :, base + s].clone()
    return flagged


def cache_tensors(cache):
    """The K and V tensors of every layer of a transformers-5 cache (or of a tuple cache)."""
    if isinstance(cache, tuple):
        return [t for layer in cache for t in layer]
    return [t for layer in cache.layers for t in (layer.keys, layer.values)]


def compact_cache(cache, path, count, base, num_slots, node_slot=None, new_length=None):
    """utils.caching.compact_cache on the host model: the move, then the length — crop for a
    DynamicCache, ``cumulative_length`` for a StaticCache, sliced views for a tuple."""
    compact(cache_tensors(cache), path, count, base, num_slots, node_slot)
    if isinstance(cache, tuple):
        return tuple(tuple(t[:, :, :new_length] for t in layer) for layer in cache)
    lens = [getattr(layer, "cumulative_length", None) for layer in cache.layers]
    if all(torch.is_tensor(t) for t in lens):
        for t in lens:
            t.fill_(new_length)
    else:
        drop = cache.layers[0].keys.shape[2] - new_length
        if drop > 0:
            cache.crop(-drop)
    return cache
