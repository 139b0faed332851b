"""Dynamic-tree speculative sampling loop (batch 1, uncached).

``tree_speculative_generate(children="topk")`` verifies the same static ``TokenTree`` at every step.
Here the tree follows the drafter (EAGLE-2): at each level only the ``width`` best nodes by cumulative
drafter log-probability are expanded, every candidate goes to a pool, and the ``num_nodes`` best of the
pool are sent to the target.  The topology never reaches the host: ``sd_tree_grow`` picks the children
and the next frontier on the device, the drafter's masks are built from its ``frontier_parent_rank``
output with torch ops, ``sd_tree_select`` emits the parents, depths and ancestor bit sets the target's
mask is built from, and ``sd_verify_tree_dynamic`` walks the per-sequence topology from device memory.
The chosen nodes are a deterministic function of the prefix, so the distinct-children rule of §4f
keeps the target's distribution exactly.  One host read per step, as in the tree loop.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import _user_process, proc_spec, sample_rows, tree_grow, tree_pool, tree_select, verify_tree_dynamic
from ..tree import DynamicTreeSpec, dynamic_attention_inputs
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor


def _draft_inputs(prefix_len: int, allow_nodes: torch.Tensor, node_depth: torch.Tensor, dtype):
    """(mask [1, 1, L, L], position_ids [1, L]) of a drafter forward over prefix + the M frontier nodes fed
    so far: allow_nodes bool [M, M] (entry (i, j): node j is node i or an ancestor of it), node_depth
    int64 [M] (1-based).  All on the device."""
    M, dev = allow_nodes.shape[0], allow_nodes.device
    L = prefix_len + M
    allow = torch.zeros(L, L, dtype=torch.bool, device=dev)
    allow[:prefix_len, :prefix_len] = torch.ones(prefix_len, prefix_len, dtype=torch.bool, device=dev).tril()
    allow[prefix_len:, :prefix_len] = True
    allow[prefix_len:, prefix_len:] = allow_nodes
    mask = torch.zeros(L, L, dtype=dtype, device=dev)
    mask.masked_fill_(~allow, torch.finfo(dtype).min)
    pos = torch.cat([torch.arange(prefix_len, device=dev), prefix_len + node_depth - 1])
    return mask[None, None], pos[None]


def _grow_tree(drafter, input_ids, cur: int, sp: DynamicTreeSpec, d_dtype, err):
    """The pool of one step: one drafter forward and one ``tree_grow`` per level, no host read."""
    dev = input_ids.device
    pool = tree_pool(1, sp.pool_size, dev)
    fed_tok = torch.empty(0, dtype=torch.long, device=dev)          # the frontier nodes fed so far, level by level
    allow = torch.zeros(0, 0, dtype=torch.bool, device=dev)
    depth = torch.empty(0, dtype=torch.long, device=dev)
    front, off = None, 0                                            # the last frontier and its first row among the fed
    for level in range(1, sp.levels + 1):
        if level == 1:
            logits = drafter(input_ids=input_ids[:, :cur], use_cache=False).logits[0]
            rows = logits[cur - 1:cur][None]
        else:
            F, M = front.token.shape[1], fed_tok.shape[0]
            # the new nodes see what their parents see (children of the root: nothing) and themselves
            new = torch.zeros(F, M + F, dtype=torch.bool, device=dev)
            if level > 2:
                new[:, :M] = allow.index_select(0, off + front.parent_rank[0].long())
            new[:, M:] = torch.eye(F, dtype=torch.bool, device=dev)
            allow = torch.cat([torch.cat([allow, torch.zeros(M, F, dtype=torch.bool, device=dev)], 1), new], 0)
            fed_tok = torch.cat([fed_tok, front.token[0]])
            depth = torch.cat([depth, torch.full((F,), level - 1, dtype=torch.long, device=dev)])
            off = M
            mask, pos = _draft_inputs(cur, allow, depth, d_dtype)
            seq = torch.cat([input_ids[0, :cur], fed_tok])[None]
            logits = drafter(input_ids=seq, attention_mask=mask, position_ids=pos, use_cache=False).logits[0]
            rows = logits[cur + off:cur + off + F][None]
        front = tree_grow(rows, level, sp.width, sp.branch, pool, None if level == 1 else front.pool, status_or=err)
    return pool


@torch.no_grad()
def dynamic_tree_speculative_generate(
    inputs: List[int],
    drafter: Module,
    target: Module,
    tokenizer=None,
    gamma: int = 5,
    logits_processor: LogitsProcessor = GreedyProcessor(),
    max_gen_len: int = 40,
    eos_tokens_id: int | List[int] = 1,
    pad_token_id: int = 0,
    first_target: bool = True,
    debug: bool = False,
    spec: Optional[DynamicTreeSpec] = None,
    trace: Optional[list] = None,
) -> Tuple[List[int], float]:
    """``tree_speculative_generate(children="topk")`` with a context-dependent tree per step; returns
    (tokens, accepted / speculated drafts with the spec's levels speculated per step).

    spec: a ``DynamicTreeSpec(levels, width, branch, num_nodes)`` (default: the single chain of ``gamma``
    levels).  Near the end of the sequence levels and num_nodes shrink to what fits.  Uncached, batch 1.
    The growth scores are the drafter's plain log-softmax (no processor); the verify runs
    ``logits_processor`` on the target rows.  The loop always uses its own ``PhiloxNoise``, seeded from
    torch's default generator.  A processor that overrides ``_process``, ``sample`` or ``__call__`` raises
    TypeError.  trace: a list that receives per step ``dict(cur, offset, parent, draft_tokens, depth, n,
    path, x, sibling_rejects)``."""
    pspec = proc_spec(logits_processor)            # TypeError for __call__ / sample overrides
    if _user_process(logits_processor) is not None:
        raise TypeError(f"unsupported logits processor {type(logits_processor).__name__}: the tree verify "
                        "fuses the rows' processing and cannot run a user _process")
    if spec is None:
        g = max(1, min(int(gamma), _lib.SD_MAX_GAMMA))
        spec = DynamicTreeSpec(g, 1, 1, g)
    elif not isinstance(spec, DynamicTreeSpec):
        spec = DynamicTreeSpec(*spec)
    noise = PhiloxNoise()
    dev = target.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError(f"specdec_amd.dynamic_tree_speculative_generate runs on the GPU (HIP); the target is on "
                           f"{dev}. There is no CPU path.")
    if torch.device(drafter.device) != torch.device(dev):
        raise RuntimeError("dynamic_tree_speculative_generate needs the drafter on the target's device")
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

    def plain_step():
        """One token from the target's row at the last position (the first token; the last position)."""
        nonlocal cur
        logits = target(input_ids=input_ids[:, :cur], use_cache=False).logits
        sample_rows(logits[:1, -1, :], pspec, noise, tokens_out=input_ids[0, cur:cur + 1], status_or=err)
        t, bits = torch.stack([input_ids[0, cur], err[0].long()]).tolist()
        _lib.raise_row_error(bits, "dynamic_tree_speculative_generate")
        cur += 1
        return t

    if first_target:
        if plain_step() in stops:
            return input_ids[0, prompt_len:cur].tolist(), 0

    specs = {}
    while cur < total_len:
        fit = total_len - cur - 1                  # drafts that still fit before the sampled token
        if fit <= 0:
            if plain_step() in stops:
                return input_ids[0, prompt_len:cur].tolist(), rate()
            continue
        levels = min(spec.levels, fit)
        if levels not in specs:
            specs[levels] = spec.truncated(levels)
        sp = specs[levels]
        N = sp.num_nodes
        pool = _grow_tree(drafter, input_ids, cur, sp, d_dtype, err)
        sel = tree_select(pool, N, sp.pool_size, status_or=err)
        mask, pos = dynamic_attention_inputs(sel.anc, sel.depth, cur, t_dtype)
        seq = torch.cat([input_ids[:, :cur], sel.tokens], 1)
        tlogits = target(input_ids=seq, attention_mask=mask, position_ids=pos, use_cache=False).logits[0]
        speculated += levels
        offset = noise.offset
        out = verify_tree_dynamic(tlogits[cur - 1:cur + N][None], sel.tokens, sel.parent, pspec, noise, levels,
                                  stop_tokens=stop_t, status_or=err, pad_token_id=pad_token_id)
        input_ids[0, cur:cur + levels + 1] = out.tokens_out[0]         # the path's tokens, x, pad
        n, x, status, stop_index, rejects, bits = (int(v) for v in torch.stack([
            out.n_accepted[0].long(), out.next_token[0], out.row_status[0].long(), out.stop_index[0].long(),
            out.n_sibling_rejects[0].long(), err[0].long()]).tolist())
        _lib.raise_row_error(bits | status, "dynamic_tree_speculative_generate")
        accepted += n
        if trace is not None:
            trace.append(dict(cur=cur, offset=offset, parent=sel.parent[0].tolist(), draft_tokens=sel.tokens[0].cpu(),
                              depth=sel.depth[0].tolist(), n=n, path=out.path[0, :n].tolist(), x=x,
                              sibling_rejects=rejects))
        if status & _lib.SD_ROW_STOP_IN_DRAFTS:
            return input_ids[0, prompt_len:cur + stop_index + 1].tolist(), rate()
        if debug:
            print(f"[specdec] pos {cur}: accepted {n}/{levels} of {N} nodes ({rejects} sibling rejects), next {x}")
        cur += n + 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), rate()
    return input_ids[0, prompt_len:].tolist(), rate()
