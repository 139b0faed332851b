"""Multi-draft speculative sampling loop (batch 1, K draft chains per step).

``speculative_generate`` verifies one drafted continuation per target forward.  Here the drafter
draws ``num_drafts`` independent continuations of γ' tokens — K batch rows of ordinary drafter
forwards, each row's draws keyed independently — the target scores all of them in ONE forward at
batch K, and ONE ``sd_verify_multi`` call walks the prefix tree of the chains by recursive rejection
sampling (SpecInfer's multi-step speculative sampling).  The emitted tokens keep the target's
distribution exactly (multi-draft verification) while more drafts are accepted per target
forward.  No tree attention is needed, so every model the batch-1 loop drives works here.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import _user_process, proc_spec, sample_rows, verify_multi
from ..utils.caching import prune_cache
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor
from .speculative_decoding import _forward, _speculative_generate


def _select_chain(cache, winner: int, K: int, dev):
    """Every batch row of the cache becomes the winner's (the chains share its prefix from here)."""
    if not (hasattr(cache, "batch_select_indices") and hasattr(cache, "crop")):
        raise ValueError("Unsupported cache type.")
    cache.batch_select_indices(torch.full((K,), winner, dtype=torch.long, device=dev))


@torch.no_grad()
def multidraft_speculative_generate(
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
    num_drafts: int = 2,
    trace: Optional[list] = None,
) -> Tuple[List[int], float]:
    """``speculative_generate`` with ``num_drafts`` draft chains per step; returns (tokens, accepted /
    speculated drafts with γ' speculated per step, so the rate compares with ``speculative_generate``).

    The loop ALWAYS uses its own ``PhiloxNoise``, seeded from torch's default generator (so it is
    deterministic under ``torch.manual_seed``), whatever ``set_noise_mode`` says: the reference
    defines no torch-generator stream order for this step.  ``num_drafts=1`` returns exactly what
    ``speculative_generate`` returns under ``set_noise_mode("philox", seed)`` with that seed.
    Per step γ' = min(gamma, 64 // num_drafts, 32, positions left).  With ``use_cache`` the caches
    must offer ``batch_select_indices`` and ``crop`` (transformers' DynamicCache does);
    ``static_cache`` is honoured for ``num_drafts=1`` only.  A processor that overrides ``_process``,
    ``sample`` or ``__call__`` raises TypeError.  trace: a list that receives per step
    ``dict(cur, g, offset, draft_tokens [K, g], n, winner, x, sibling_rejects)`` (not with
    ``num_drafts=1``, which runs the single-chain loop)."""
    spec = proc_spec(logits_processor)             # TypeError for __call__ / sample overrides
    if _user_process(logits_processor) is not None:
        raise TypeError(f"unsupported logits processor {type(logits_processor).__name__}: the multi-draft verify "
                        "fuses the rows' processing and cannot run a user _process")
    K = int(num_drafts)
    if not 1 <= K <= _lib.SD_MULTI_MAX_DRAFTS:
        raise ValueError(f"num_drafts must be in 1..{_lib.SD_MULTI_MAX_DRAFTS}, got {num_drafts}")
    noise = PhiloxNoise()
    if K == 1:
        return _speculative_generate(noise, inputs, drafter, target, gamma, logits_processor, max_gen_len,
                                     eos_tokens_id, pad_token_id, use_cache, False, first_target, debug, static_cache)
    if static_cache and use_cache:
        raise ValueError("Unsupported cache type.")
    dev = target.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("specdec_amd.multidraft_speculative_generate runs on the GPU (HIP); the target is on "
                           f"{dev}. There is no CPU path.")
    if torch.device(drafter.device) != torch.device(dev):
        raise RuntimeError("multidraft_speculative_generate needs the drafter on the target's device")
    stops = eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id]
    stop_t = torch.tensor(stops, dtype=torch.long, device=dev)
    accepted, speculated = 0.0, 0.0
    cfg = target.config
    max_seq = getattr(cfg, "max_position_embeddings", None) or getattr(cfg, "max_context_length", None) or 1024
    prompt_len = len(inputs)
    total_len = min(max_seq, prompt_len + max_gen_len)
    input_ids = torch.full((K, total_len), pad_token_id, dtype=torch.long, device=dev)
    input_ids[:, :prompt_len] = torch.tensor(inputs, dtype=torch.long, device=dev)
    cur = prompt_len
    drafter_cache = target_cache = None
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def rate():
        return accepted / speculated if speculated else 0

    if first_target:
        logits, target_cache, _ = _forward(target, input_ids, cur, target_cache, use_cache)
        sample_rows(logits[:1, -1, :], spec, noise, tokens_out=input_ids[0, cur:cur + 1], status_or=err)
        t, bits = torch.stack([input_ids[0, cur], err[0].long()]).tolist()
        _lib.raise_row_error(bits, "multidraft_speculative_generate")
        input_ids[1:, cur] = t
        cur += 1
        if t in stops:
            return input_ids[0, prompt_len:cur].tolist(), 0

    g_cap = min(gamma, _lib.SD_MULTI_MAX_NODES // K, _lib.SD_MAX_GAMMA)
    stash = not spec.keeps                         # as the batch-1 loop: the draws' (max, Σexp) feed the verify
    dstats = torch.empty(max(g_cap, 1), K, 2, dtype=torch.float32, device=dev) if stash else None
    while cur < total_len:
        g = min(g_cap, total_len - cur - 1)
        draft_rows = []
        for k in range(g):                         # γ' drafter forwards at batch K, one draw per chain
            logits, drafter_cache, _ = _forward(drafter, input_ids, cur + k, drafter_cache, use_cache)
            row = logits[:, -1, :].contiguous()
            tok = input_ids[:, cur + k]
            sample_rows(row, spec, noise, tokens_out=tok, row_stats_out=dstats[k] if stash else None, status_or=err)
            tok.clamp_(0, row.shape[-1] - 1)       # a failed row's -1 never reaches a forward
            draft_rows.append(row)
        speculated += g
        logits, target_cache, start = _forward(target, input_ids, cur + g, target_cache, use_cache)
        if g == 0:                                 # last position: the bonus row is sampled
            sample_rows(logits[:1, cur - 1 - start, :], spec, noise, tokens_out=input_ids[0, cur:cur + 1],
                        status_or=err)
            x, bits = torch.stack([input_ids[0, cur], err[0].long()]).tolist()
            _lib.raise_row_error(bits, "multidraft_speculative_generate")
            cur += 1
            if x in stops:
                return input_ids[0, prompt_len:cur].tolist(), rate()
            continue
        trows = [logits[:, cur - 1 + t - start, :] for t in range(g + 1)]
        drafts = input_ids[:, cur:cur + g]
        offset = noise.offset
        out = verify_multi(trows, draft_rows, drafts, spec, noise, num_drafts=K, stop_tokens=stop_t,
                           draft_row_stats=dstats[:g] if stash else None, status_or=err, pad_token_id=pad_token_id)
        kept = drafts.clone() if trace is not None else None
        input_ids[:, cur:cur + g + 1] = out.tokens_out[0]              # tok[winner, :n], x, pad — every row
        n, winner, x, status, stop_index, rejects, bits = (int(v) for v in torch.stack([
            out.n_accepted[0].long(), out.winner[0].long(), out.next_token[0], out.row_status[0].long(),
            out.stop_index[0].long(), out.n_sibling_rejects[0].long(), err[0].long()]).tolist())
        _lib.raise_row_error(bits | status, "multidraft_speculative_generate")
        accepted += n
        if trace is not None:
            trace.append(dict(cur=cur, g=g, offset=offset, draft_tokens=kept.cpu(), n=n, winner=winner, x=x,
                              sibling_rejects=rejects))
        if status & _lib.SD_ROW_STOP_IN_DRAFTS:
            return input_ids[0, prompt_len:cur + stop_index + 1].tolist(), rate()
        if use_cache:
            _select_chain(drafter_cache, winner, K, dev)
            _select_chain(target_cache, winner, K, dev)
            if n < g:
                drafter_cache = prune_cache(drafter_cache, g - n)
                target_cache = prune_cache(target_cache, g - n + 1)
        if debug:
            print(f"[specdec] pos {cur}: accepted {n}/{g} (chain {winner}, {rejects} sibling rejects), next {x}")
        cur += n + 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), rate()
    return input_ids[0, prompt_len:].tolist(), rate()
