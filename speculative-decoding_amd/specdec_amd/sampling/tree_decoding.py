"""Token-tree speculative sampling loop (batch 1, one tree of drafted nodes per step).

``multidraft_speculative_generate`` verifies K equal chains and runs the target at batch K.  Here the
drafter grows a ``TokenTree`` level by level — tree-masked forwards over prefix + the nodes so far, the
children of a node drawn as independent samples of that node's row — the target scores the whole tree
in ONE batch-1 forward under the tree attention mask (a 4-D additive mask and ``position_ids``), and
ONE ``sd_verify_tree`` call walks it by recursive rejection sampling.  The emitted tokens keep the
target's distribution exactly while the tree puts its width where rejections happen.
The models must honour a 4-D additive ``attention_mask`` and ``position_ids`` (transformers' do).

With ``use_cache=True`` both models keep a KV cache and every forward feeds only the tokens the cache
lacks ("Cached loop"): the target the root and the N nodes, the drafter the nodes of
the level before.  After the verify ONE ``sd_kv_compact`` launch per cache moves the accepted path's
entries from their scattered positions ``cur + slot(path[d])`` to ``cur + d`` in every layer, driven
by the verify's device outputs (``utils.caching.compact_cache``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import _user_process, proc_spec, sample_rows, topk_children, verify_tree, verify_tree_distinct
from ..tree import TokenTree
from ..utils.caching import DynamicCache, _static_lengths, compact_cache
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor


def _tree_forward(model, seq: torch.Tensor, tree: TokenTree, prefix_len: int, n_nodes: int, dtype):
    """Logits [L, V] of `model` over prefix + the first n_nodes nodes of the tree under its mask."""
    mask, pos = tree.attention_inputs(prefix_len, dtype, seq.device, num_nodes=n_nodes)
    out = model(input_ids=seq[:, :prefix_len + n_nodes], attention_mask=mask, position_ids=pos, use_cache=False)
    return out.logits[0]


def _allowed(tr: TokenTree, cur: int, start: int, nodes, col_of) -> Tuple[torch.Tensor, torch.Tensor]:
    """(allow bool [R, cols], position_ids [1, R]) of a cached forward that feeds the committed tokens
    [start, cur) and then `nodes`: the rows of ``TokenTree.attention_inputs`` that belong to the new
    tokens, over the cache's columns.  Committed rows are causal; a node sees the committed tokens, its
    ancestors and itself, node j lying in column cur + col_of[j].  cols ends with the last new token."""
    m = cur - start
    cols = cur + (max(col_of[i] for i in nodes) + 1 if nodes else 0)
    allow = torch.zeros(m + len(nodes), cols, dtype=torch.bool)
    allow[:m, :cur] = torch.ones(m, cur, dtype=torch.bool).tril(diagonal=start)
    for r, i in enumerate(nodes):
        allow[m + r, :cur] = True
        allow[m + r, [cur + col_of[j] for j in tr.path_to(i)]] = True
    pos = list(range(start, cur)) + [cur + tr.node_depth[i] - 1 for i in nodes]
    return allow, torch.tensor([pos], dtype=torch.long)


class _CachedModel:
    """A model, its KV cache and the host's copy of the cache length (the loop keeps one integer per
    model; a StaticCache's own length is a device tensor).  width: a StaticCache's max_cache_len, or
    None for the DynamicCache the model's first forward returns."""

    def __init__(self, model, dtype, width: Optional[int], dev):
        self.model, self.dtype, self.width, self.dev = model, dtype, width, dev
        self.cache, self.len = None, 0
        if width is not None:
            from transformers.cache_utils import StaticCache
            self.cache = StaticCache(config=model.config, max_cache_len=width)

    def forward(self, tokens: torch.Tensor, allow: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None):
        """Logits [R, V] of the R new `tokens` [1, R], appended to the cache at [len, len + R).  allow /
        pos: from _allowed; None is the plain causal forward."""
        R = tokens.shape[1]
        kw = {}
        if allow is not None:
            mask = torch.full((R, self.width or self.len + R), torch.finfo(self.dtype).min, dtype=self.dtype)
            mask[:, :self.len + R].masked_fill_(allow, 0)          # a StaticCache's tail stays masked
            kw.update(attention_mask=mask[None, None].to(self.dev), position_ids=pos.to(self.dev))
        if self.width is not None:
            kw["cache_position"] = torch.arange(self.len, self.len + R, device=self.dev)
        out = self.model(input_ids=tokens, past_key_values=self.cache, use_cache=True, **kw)
        got = getattr(out, "past_key_values", None)
        if self.width is not None:
            ok = got is self.cache and _static_lengths(got) is not None
        else:
            ok = DynamicCache is not None and isinstance(got, DynamicCache)
        if not ok:
            raise ValueError("Unsupported cache type.")
        self.cache = got
        self.len += R
        return out.logits[0]

    def compact(self, path, count, base: int, num_slots: int, node_slot, new_length: int) -> None:
        """The cache onto the accepted path: positions base + slot(path[d]) -> base + d, length new_length
        (a StaticCache's is set from `count` on the device)."""
        if num_slots > 0:
            self.cache = compact_cache(self.cache, path, count, base, num_slots=num_slots, node_slot=node_slot,
                                       new_length=None if self.width is not None else new_length)
        self.len = new_length


def _topk_level(logits: torch.Tensor, row_of, tr: TokenTree, level) -> torch.Tensor:
    """The tokens of a level's nodes under ``children="topk"``: ONE ``topk_children`` call over the rows
    of the level's distinct parent slots (row_of: slot -> row of `logits`), k the level's largest child
    count; child j of a slot, in ascending node index, gets the slot's (j+1)-th best token."""
    slots = sorted({tr.parent[c] + 1 for c in level})
    dev, V = logits.device, logits.shape[-1]
    k = min(max(len(tr.children[s]) for s in slots), V)
    at = torch.tensor([row_of[s] for s in slots], dtype=torch.long, device=dev)
    best = topk_children(logits.index_select(0, at), k)
    r = [slots.index(tr.parent[c] + 1) for c in level]
    j = [min(tr.children[tr.parent[c] + 1].index(c), k - 1) for c in level]    # k < child count only where V is
    return best[torch.tensor(r, dtype=torch.long, device=dev), torch.tensor(j, dtype=torch.long, device=dev)]


def _cached_rows(tm: _CachedModel, dm: _CachedModel, tr: TokenTree, cur: int, input_ids, spec, noise, err, pad_token_id,
                 children: str = "sample"):
    """One step's drafting and target forward on the caches: the uncached loop's draws (one sample_rows call
    per level, the parent's row once per child) on rows of forwards over the new tokens only.  Returns
    (target rows [1, N + 1, V], drafter rows by slot, drafts [1, N], slot), slot[i] the order in which node i
    entered the drafter's cache (-1: the deepest level, never fed)."""
    N, dev = tr.num_nodes, tm.dev
    slot = [-1] * N
    for k, i in enumerate(i for level in tr.levels[:-1] for i in level):
        slot[i] = k
    drafts = torch.full((1, N), pad_token_id, dtype=torch.long, device=dev)
    draft_rows = [None] * (N + 1)
    for k, level in enumerate(tr.levels):
        if k == 0:                                         # the committed tokens the cache lacks; the root's row is last
            logits = dm.forward(input_ids[:, dm.len:cur])
            row_of = {0: logits.shape[0] - 1}
        else:                                              # the nodes of the level before, under their ancestor mask
            prev = tr.levels[k - 1]
            allow, pos = _allowed(tr, cur, cur, prev, slot)
            logits = dm.forward(drafts[:, prev], allow, pos)
            row_of = {i + 1: r for r, i in enumerate(prev)}
        for s in sorted({tr.parent[c] + 1 for c in level}):
            draft_rows[s] = logits[row_of[s]:row_of[s] + 1, :]
        if children == "topk":
            toks = _topk_level(logits, row_of, tr, level)
        else:
            at = torch.tensor([row_of[tr.parent[c] + 1] for c in level], dtype=torch.long, device=dev)
            rows = logits.index_select(0, at)
            toks = torch.empty(len(level), dtype=torch.long, device=dev)
            sample_rows(rows, spec, noise, tokens_out=toks, status_or=err)
            toks.clamp_(0, rows.shape[-1] - 1)             # a failed row's -1 never reaches a forward
        drafts[0, torch.tensor(level, dtype=torch.long, device=dev)] = toks
    m = cur - tm.len                                       # committed tokens the target's cache lacks (the root is last)
    allow, pos = _allowed(tr, cur, tm.len, list(range(N)), list(range(N)))
    tlogits = tm.forward(torch.cat([input_ids[:, tm.len:cur], drafts], 1), allow, pos)
    return tlogits[m - 1:m + N][None], draft_rows, drafts, slot


@torch.no_grad()
def tree_speculative_generate(
    inputs: List[int],
    drafter: Module,
    target: Module,
    tokenizer=None,
    gamma: int = 5,
    logits_processor: LogitsProcessor = GreedyProcessor(),
    max_gen_len: int = 40,
    eos_tokens_id: int | List[int] = 1,
    pad_token_id: int = 0,
    use_cache: bool = False,
    first_target: bool = True,
    debug: bool = False,
    static_cache: bool = False,
    tree: Optional[TokenTree] = None,
    trace: Optional[list] = None,
    children: str = "sample",
) -> Tuple[List[int], float]:
    """``speculative_generate`` with a token tree per step; returns (tokens, accepted / speculated
    drafts with the tree's depth speculated per step, so the rate compares with
    ``speculative_generate`` at γ = depth).

    tree: a ``TokenTree`` (default ``TokenTree.chains(1, gamma)``, the single chain).  Near the end of
    the sequence the tree is truncated to the depth that still fits.  The loop ALWAYS uses its own
    ``PhiloxNoise``, seeded from torch's default generator (so it is deterministic under
    ``torch.manual_seed``), whatever ``set_noise_mode`` says.  ``use_cache=True`` runs the cached loop:
    each model keeps a DynamicCache, or with ``static_cache=True`` a StaticCache of
    total_len + tree.num_nodes positions, compacted onto the accepted path after every verify; the
    draws and the noise are the uncached loop's.  A model whose forward returns no cache or another
    cache type raises ValueError("Unsupported cache type."), as does ``static_cache`` without
    ``use_cache``.  A processor that overrides ``_process``, ``sample`` or ``__call__`` raises
    TypeError.  trace: a list that receives per step ``dict(cur, offset, parent, draft_tokens [N], n,
    path, x, sibling_rejects)``, and under ``use_cache`` the cache lengths at the step's start,
    ``cache_len_target`` and ``cache_len_drafter``.

    children: "sample" (the default) draws the children of a slot as iid samples of the slot's drafter
    row and verifies with ``sd_verify_tree``.  "topk" gives child j of a slot the slot's (j+1)-th best
    drafter token (one ``topk_children`` call per level) and verifies with ``sd_verify_tree_distinct``
    (DESIGN.md §4f): distinct candidates, no drafter rows in the verify, and under greedy exactly the
    target's greedy decode.  Pick "topk" for greedy and for peaked drafters, "sample" for flat ones."""
    if children not in ("sample", "topk"):
        raise ValueError(f"children must be 'sample' or 'topk', got {children!r}")
    topk = children == "topk"
    spec = proc_spec(logits_processor)             # TypeError for __call__ / sample overrides
    if _user_process(logits_processor) is not None:
        raise TypeError(f"unsupported logits processor {type(logits_processor).__name__}: the tree verify "
                        "fuses the rows' processing and cannot run a user _process")
    if static_cache and not use_cache:
        raise ValueError("Unsupported cache type.")
    if tree is None:
        tree = TokenTree.chains(1, max(1, min(int(gamma), _lib.SD_MAX_GAMMA)))
    elif not isinstance(tree, TokenTree):
        tree = TokenTree(tree)
    noise = PhiloxNoise()
    dev = target.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError(f"specdec_amd.tree_speculative_generate runs on the GPU (HIP); the target is on {dev}. "
                           "There is no CPU path.")
    if torch.device(drafter.device) != torch.device(dev):
        raise RuntimeError("tree_speculative_generate needs the drafter on the target's device")
    stops = eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id]
    stop_t = torch.tensor(stops, dtype=torch.long, device=dev)
    accepted, speculated = 0.0, 0.0
    cfg = target.config
    max_seq = getattr(cfg, "max_position_embeddings", None) or getattr(cfg, "max_context_length", None) or 1024
    prompt_len = len(inputs)
    total_len = min(max_seq, prompt_len + max_gen_len)
    input_ids = torch.full((1, total_len), pad_token_id, dtype=torch.long, device=dev)
    input_ids[0, :prompt_len] = torch.tensor(inputs, dtype=torch.long, device=dev)
    cur = prompt_len
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    t_dtype = getattr(target, "dtype", None) or torch.float32
    d_dtype = getattr(drafter, "dtype", None) or torch.float32

    def rate():
        return accepted / speculated if speculated else 0

    if use_cache:
        width = total_len + tree.num_nodes if static_cache else None
        tm, dm = _CachedModel(target, t_dtype, width, dev), _CachedModel(drafter, d_dtype, width, dev)

    def plain_step():
        """One token from the target's row at the last position (the first token; the last position)."""
        nonlocal cur
        if use_cache:                              # the tokens the target's cache lacks
            logits = tm.forward(input_ids[:, tm.len:cur])[None]
        else:
            logits = target(input_ids=input_ids[:, :cur], use_cache=False).logits
        sample_rows(logits[:1, -1, :], spec, noise, tokens_out=input_ids[0, cur:cur + 1], status_or=err)
        t, bits = torch.stack([input_ids[0, cur], err[0].long()]).tolist()
        _lib.raise_row_error(bits, "tree_speculative_generate")
        cur += 1
        return t

    if first_target:
        if plain_step() in stops:
            return input_ids[0, prompt_len:cur].tolist(), 0

    trees = {}
    while cur < total_len:
        fit = total_len - cur - 1                  # drafts that still fit before the sampled token
        if fit <= 0:
            if plain_step() in stops:
                return input_ids[0, prompt_len:cur].tolist(), rate()
            continue
        depth = min(tree.depth, fit)
        if depth not in trees:
            trees[depth] = tree.truncated(depth)
        tr = trees[depth]
        N = tr.num_nodes
        if use_cache:
            t_len, d_len = tm.len, dm.len
            target_rows, draft_rows, drafts, slot = _cached_rows(tm, dm, tr, cur, input_ids, spec, noise, err, pad_token_id,
                                                                 children)
        else:
            seq = torch.cat([input_ids[:, :cur], torch.full((1, N), pad_token_id, dtype=torch.long, device=dev)], 1)
            draft_rows = [None] * (N + 1)
            placed = 0                                 # nodes whose tokens are drawn: those of the levels so far
            for level in tr.levels:                    # one drafter forward and one draw per level
                logits = _tree_forward(drafter, seq, tr, cur, placed, d_dtype)
                slots = sorted({tr.parent[c] + 1 for c in level})
                for s in slots:
                    draft_rows[s] = logits[cur - 1 + s:cur + s, :]
                if topk:
                    toks = _topk_level(logits, {s: cur - 1 + s for s in slots}, tr, level)
                else:
                    # the parent's row once per child: every child is an independent draw (its own noise row)
                    at = torch.tensor([cur - 1 + tr.parent[c] + 1 for c in level], dtype=torch.long, device=dev)
                    rows = logits.index_select(0, at)
                    toks = torch.empty(len(level), dtype=torch.long, device=dev)
                    sample_rows(rows, spec, noise, tokens_out=toks, status_or=err)
                    toks.clamp_(0, rows.shape[-1] - 1) # a failed row's -1 never reaches a forward
                seq[0, cur + torch.tensor(level, dtype=torch.long, device=dev)] = toks
                placed = max(placed, max(level) + 1)
            tlogits = _tree_forward(target, seq, tr, cur, N, t_dtype)
            drafts = seq[:, cur:cur + N].contiguous()
            target_rows = tlogits[cur - 1:cur + N][None]
        speculated += depth
        offset = noise.offset
        if topk:
            out = verify_tree_distinct(target_rows, drafts, tr, spec, noise, stop_tokens=stop_t, status_or=err,
                                       pad_token_id=pad_token_id)
        else:
            out = verify_tree(target_rows, draft_rows, drafts, tr, spec, noise, stop_tokens=stop_t,
                              status_or=err, pad_token_id=pad_token_id)
        input_ids[0, cur:cur + depth + 1] = out.tokens_out[0]          # the path's tokens, x, pad
        n, x, status, stop_index, rejects, bits = (int(v) for v in torch.stack([
            out.n_accepted[0].long(), out.next_token[0], out.row_status[0].long(), out.stop_index[0].long(),
            out.n_sibling_rejects[0].long(), err[0].long()]).tolist())
        _lib.raise_row_error(bits | status, "tree_speculative_generate")
        accepted += n
        if trace is not None:
            trace.append(dict(cur=cur, offset=offset, parent=list(tr.parent), draft_tokens=drafts[0].cpu(), n=n,
                              path=out.path[0, :n].tolist(), x=x, sibling_rejects=rejects))
            if use_cache:
                trace[-1].update(cache_len_target=t_len, cache_len_drafter=d_len)
        if status & _lib.SD_ROW_STOP_IN_DRAFTS:
            return input_ids[0, prompt_len:cur + stop_index + 1].tolist(), rate()
        if use_cache:
            # the caches onto the accepted path, by the verify's device outputs.  The target holds every node at
            # cur + i; the drafter lacks the deepest level, so a fully accepted path leaves its last node to the
            # next step's first forward.
            fed = sum(s >= 0 for s in slot)
            tm.compact(out.path, out.n_accepted, cur, N, None, cur + n)
            dm.compact(out.path, out.n_accepted.clamp(max=depth - 1), cur, fed, slot, cur + min(n, depth - 1))
        if debug:
            print(f"[specdec] pos {cur}: accepted {n}/{depth} of {N} nodes ({rejects} sibling rejects), next {x}")
        cur += n + 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), rate()
    return input_ids[0, prompt_len:].tolist(), rate()
