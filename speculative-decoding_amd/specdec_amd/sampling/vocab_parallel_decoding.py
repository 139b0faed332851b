"""Speculative sampling loop (batch 1) for a tensor-parallel target whose LM head is column-parallel:
every rank ends the target forward with a vocabulary slice [1, L, V_s] of the logits, and the verify
step runs on the slices (``verify_vocab_parallel``: two exchanges of a few hundred bytes per step; the
logit rows are never gathered).

The drafter is replicated: every rank runs it on the same ids and draws the same drafts with
``sample_rows`` on the same Philox offsets, then passes its slice of the drafter's full rows to the
verify.  It is ``speculative_generate``'s loop without the KV cache (every forward sees the whole
prefix); cache handling for a sharded target is the serving stack's.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import sample_rows
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor
from ..vocab_parallel import LocalShards, VocabShard, _vp_spec, verify_vocab_parallel


@torch.no_grad()
def vocab_parallel_speculative_generate(
    inputs: List[int],
    drafter: Module,
    target_shard_fn: Union[Callable, Sequence[Callable]],
    shard: Optional[VocabShard],
    exchange,
    gamma: int = 5,
    logits_processor: LogitsProcessor = GreedyProcessor(),
    max_gen_len: int = 40,
    eos_tokens_id: int | List[int] = 1,
    pad_token_id: int = 0,
    first_target: bool = True,
    seed: Optional[int] = None,
    trace: Optional[list] = None,
) -> Tuple[List[int], float]:
    """``speculative_generate`` on a vocabulary-sharded target; returns (tokens, accepted / speculated).

    target_shard_fn(input_ids [1, L]) -> logits [1, L, V_s]: this rank's columns
    [shard.vocab_offset, + shard.vocab_local) of the tensor-parallel target's logits.  drafter: the
    replicated drafter model (full rows).  exchange: the all-gather of one block per rank
    (``GroupExchange``).  seed: the loop's PhiloxNoise seed — EVERY RANK MUST PASS THE SAME (None draws
    it from torch's default generator: seed that alike on every rank).  The logits processor is greedy
    or multinomial at any temperature; a user ``_process`` or any other processor raises TypeError (the
    vocabulary-parallel verify has no top-k / nucleus search over slices).  trace: a list that
    receives per step ``(offset, draft tokens, n, x, status)`` (the first-target token is a step with
    no drafts).  Every rank returns the same tokens.

    Single-GPU emulation: with ``exchange`` a ``LocalShards``, target_shard_fn is one function per
    shard (shard=None) and the S shards' steps run in lock step in this process."""
    spec = _vp_spec(logits_processor)
    emu = isinstance(exchange, LocalShards)
    if emu:
        fns = list(target_shard_fn) if not callable(target_shard_fn) else None
        if fns is None or len(fns) != len(exchange.shards):
            raise ValueError("with LocalShards, target_shard_fn is one function per shard")
        shards = exchange.shards
    else:
        if not isinstance(shard, VocabShard):
            raise TypeError("shard must be a VocabShard")
        fns, shards = [target_shard_fn], [shard]
    dev = torch.device(drafter.device)
    if dev.type != "cuda":
        raise RuntimeError(f"vocab_parallel_speculative_generate runs on the GPU (HIP); the drafter is on {dev}. "
                           "There is no CPU path.")
    noise = PhiloxNoise(seed)
    stops = eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id]
    stop_t = torch.tensor(stops, dtype=torch.long, device=dev)
    cfg = drafter.config
    max_seq = getattr(cfg, "max_position_embeddings", None) or getattr(cfg, "max_context_length", None) or 1024
    prompt_len = len(inputs)
    total_len = min(max_seq, prompt_len + max_gen_len)
    input_ids = torch.full((1, total_len), pad_token_id, dtype=torch.long, device=dev)
    input_ids[0, :prompt_len] = torch.tensor(inputs, dtype=torch.long, device=dev)
    cur = prompt_len
    accepted, speculated = 0.0, 0.0
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def rate():
        return accepted / speculated if speculated else 0

    def target_slices(end: int, first_row: int):
        """Per shard: rows first_row.. of the target's slice logits on ids[:, :end] (views)."""
        out = []
        for fn, sh in zip(fns, shards):
            logits = fn(input_ids[:, :end])
            if logits.dim() != 3 or logits.shape[0] != 1 or logits.shape[1] != end or logits.shape[2] != sh.vocab_local:
                raise ValueError(f"target_shard_fn must return [1, {end}, {sh.vocab_local}], got {tuple(logits.shape)}")
            out.append(logits[:, first_row:, :])
        return out

    def step(ts, ds, drafts):
        offset = noise.offset
        if emu:
            out = verify_vocab_parallel(ts, ds, drafts, spec, noise, None, exchange, stop_tokens=stop_t, status_or=err)[0]
        else:
            out = verify_vocab_parallel(ts[0], ds[0] if ds else None, drafts, spec, noise, shard, exchange,
                                        stop_tokens=stop_t, status_or=err)
        n, x, status, stop_index, bits = (int(v) for v in torch.stack([
            out.n_accepted[0].long(), out.next_token[0], out.row_status[0].long(), out.stop_index[0].long(),
            err[0].long()]).tolist())
        _lib.raise_row_error(bits | status, "vocab_parallel_speculative_generate")
        if trace is not None:
            trace.append((offset, [] if drafts is None else drafts[0].tolist(), n, x, status))
        return n, x, status, stop_index

    if first_target:                                   # γ' = 0: sample the one target row
        _, x, _, _ = step(target_slices(cur, cur - 1), None, None)
        input_ids[0, cur] = x
        cur += 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), 0

    while cur < total_len:
        g = min(gamma, _lib.SD_MAX_GAMMA, total_len - cur - 1)
        draft_rows = []
        for k in range(g):                             # the replicated drafter: the same draws on every rank
            row = drafter(input_ids=input_ids[:, :cur + k]).logits[:, -1, :]
            sample_rows(row, spec, noise, tokens_out=input_ids[0, cur + k:cur + k + 1], status_or=err)
            input_ids[0, cur + k:cur + k + 1].clamp_(0, row.shape[-1] - 1)   # a failed row's -1 never reaches a forward
            draft_rows.append(row)
        speculated += g
        ts = target_slices(cur + g, cur - 1)           # [1, g+1, V_s]: rows cur-1 .. cur-1+g
        ds = [[sh.view(r) for r in draft_rows] for sh in shards] if g else None
        drafts = input_ids[:, cur:cur + g].clone() if g else None
        n, x, status, stop_index = step(ts, ds, drafts)
        accepted += n
        if status & _lib.SD_ROW_STOP_IN_DRAFTS:
            return input_ids[0, prompt_len:cur + stop_index + 1].tolist(), rate()
        input_ids[0, cur + n] = x
        if n + 1 < g + 1:
            input_ids[0, cur + n + 1:cur + g + 1] = pad_token_id
        cur += n + 1
        if x in stops:
            return input_ids[0, prompt_len:cur].tolist(), rate()
    return input_ids[0, prompt_len:].tolist(), rate()
