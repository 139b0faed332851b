"""Token-tree speculative sampling loop (batch 1, one tree of drafted nodes per step).

``multidraft_speculative_generate`` verifies K equal chains and runs the target at batch K.  Here the
drafter grows a ``TokenTree`` level by level — tree-masked forwards over prefix + the nodes so far, the
children of a node drawn as independent samples of that node's row — the target scores the whole tree
in ONE batch-1 forward under the tree attention mask (a 4-D additive mask and ``position_ids``), and
ONE ``sd_verify_tree`` call walks it by recursive rejection sampling.  The emitted tokens keep the
target's distribution exactly while the tree puts its width where rejections happen.
The models must honour a 4-D additive ``attention_mask`` and ``position_ids`` (transformers' do).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import _user_process, proc_spec, sample_rows, verify_tree
from ..tree import TokenTree
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor


def _tree_forward(model, seq: torch.Tensor, tree: TokenTree, prefix_len: int, n_nodes: int, dtype):
    """Logits [L, V] of `model` over prefix + the first n_nodes nodes of the tree under its mask."""
    mask, pos = tree.attention_inputs(prefix_len, dtype, seq.device, num_nodes=n_nodes)
    out = model(input_ids=seq[:, :prefix_len + n_nodes], attention_mask=mask, position_ids=pos, use_cache=False)
    return out.logits[0]


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
) -> Tuple[List[int], float]:
    """``speculative_generate`` with a token tree per step; returns (tokens, accepted / speculated
    drafts with the tree's depth speculated per step, so the rate compares with
    ``speculative_generate`` at γ = depth).

    tree: a ``TokenTree`` (default ``TokenTree.chains(1, gamma)``, the single chain).  Near the end of
    the sequence the tree is truncated to the depth that still fits.  The loop ALWAYS uses its own
    ``PhiloxNoise``, seeded from torch's default generator (so it is deterministic under
    ``torch.manual_seed``), whatever ``set_noise_mode`` says.  ``use_cache=True`` raises
    ValueError("Unsupported cache type."): compacting a KV cache onto the accepted path is not part of
    this loop (``verify_tree``'s ``path`` output is what it needs).  A processor that overrides
    ``_process``, ``sample`` or ``__call__`` raises TypeError.  trace: a list that receives per step
    ``dict(cur, offset, parent, draft_tokens [N], n, path, x, sibling_rejects)``."""
    spec = proc_spec(logits_processor)             # TypeError for __call__ / sample overrides
    if _user_process(logits_processor) is not None:
        raise TypeError(f"unsupported logits processor {type(logits_processor).__name__}: the tree verify "
                        "fuses the rows' processing and cannot run a user _process")
    if use_cache or static_cache:
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

    def plain_step():
        """One token from the target's row at the last position (the first token; the last position)."""
        nonlocal cur
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
        seq = torch.cat([input_ids[:, :cur], torch.full((1, N), pad_token_id, dtype=torch.long, device=dev)], 1)
        draft_rows = [None] * (N + 1)
        placed = 0                                 # nodes whose tokens are drawn: those of the levels so far
        for level in tr.levels:                    # one drafter forward and one draw per level
            logits = _tree_forward(drafter, seq, tr, cur, placed, d_dtype)
            slots = sorted({tr.parent[c] + 1 for c in level})
            for s in slots:
                draft_rows[s] = logits[cur - 1 + s:cur + s, :]
            # the parent's row once per child: every child is an independent draw (its own noise row)
            at = torch.tensor([cur - 1 + tr.parent[c] + 1 for c in level], dtype=torch.long, device=dev)
            rows = logits.index_select(0, at)
            toks = torch.empty(len(level), dtype=torch.long, device=dev)
            sample_rows(rows, spec, noise, tokens_out=toks, status_or=err)
            toks.clamp_(0, rows.shape[-1] - 1)     # a failed row's -1 never reaches a forward
            seq[0, cur + torch.tensor(level, dtype=torch.long, device=dev)] = toks
            placed = max(placed, max(level) + 1)
        speculated += depth
        tlogits = _tree_forward(target, seq, tr, cur, N, t_dtype)
        drafts = seq[:, cur:cur + N].contiguous()
        offset = noise.offset
        out = verify_tree(tlogits[cur - 1:cur + N][None], draft_rows, drafts, tr, spec, noise, stop_tokens=stop_t,
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
        if status & _lib.SD_ROW_STOP_IN_DRAFTS:
            return input_ids[0, prompt_len:cur + stop_index + 1].tolist(), rate()
        if debug:
            print(f"[specdec] pos {cur}: accepted {n}/{depth} of {N} nodes ({rejects} sibling rejects), next {x}")
        cur += n + 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), rate()
    return input_ids[0, prompt_len:].tolist(), rate()
