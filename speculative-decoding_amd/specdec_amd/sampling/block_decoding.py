"""Block-verification speculative sampling loop (batch 1, one draft chain per step).

``speculative_generate`` tests the drafted tokens one by one and stops at the first failure.  Here the
same γ' drafter forwards and the same single target forward feed ONE ``sd_verify_block`` call, which
verifies the drafted block jointly (Sun et al., "Block Verification Accelerates Speculative Decoding"):
the emitted tokens keep the target's distribution exactly, and the expected number of accepted drafts
per target forward is never below the token-wise rule's.  Nothing else changes — no
extra forward, no tree mask — so the loop is ``speculative_generate``'s own step code with another
accept rule, cache pruning by the verify's prune outputs included.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.nn import Module

from .. import _lib
from ..noise import PhiloxNoise
from ..ops import _user_process, proc_spec, verify_block
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor
from .speculative_decoding import _speculative_generate


@torch.no_grad()
def block_speculative_generate(
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
    trace: Optional[list] = None,
) -> Tuple[List[int], float]:
    """``speculative_generate`` with the drafted block verified jointly; returns (tokens, accepted /
    speculated drafts).

    The loop ALWAYS uses its own ``PhiloxNoise``, seeded from torch's default generator (so it is
    deterministic under ``torch.manual_seed``), whatever ``set_noise_mode`` says: the rule defines no
    torch-generator stream order.  Per step γ' = min(gamma, 32, positions left).  ``gamma=1``, where the
    two rules coincide, returns exactly what ``speculative_generate`` returns under
    ``set_noise_mode("philox", seed)`` with that seed.  ``use_cache`` and ``static_cache`` crop the caches
    by the verify's prune outputs, as the chain loop.  A processor that overrides ``_process``, ``sample``
    or ``__call__`` raises TypeError.  trace: a list that receives per verify step
    ``dict(cur, g, offset, draft_tokens [g], n, x)``."""
    proc_spec(logits_processor)                    # TypeError for __call__ / sample overrides
    if _user_process(logits_processor) is not None:
        raise TypeError(f"unsupported logits processor {type(logits_processor).__name__}: the block verify "
                        "fuses the rows' processing and cannot run a user _process")
    if gamma < 1:
        raise ValueError(f"gamma must be at least 1, got {gamma}")
    if torch.device(drafter.device) != torch.device(target.device):
        raise RuntimeError("block_speculative_generate needs the drafter on the target's device")
    noise = PhiloxNoise()

    def step(target_rows, draft_rows, drafts, proc, noise, stop_tokens, draft_row_stats, status_or):
        return verify_block(target_rows, draft_rows, drafts, proc, noise, stop_tokens=stop_tokens,
                            draft_row_stats=draft_row_stats, status_or=status_or, pad_token_id=pad_token_id,
                            want_tokens=False)

    g = min(int(gamma), _lib.SD_MAX_GAMMA)
    return _speculative_generate(noise, inputs, drafter, target, g, logits_processor, max_gen_len, eos_tokens_id,
                                 pad_token_id, use_cache, False, first_target, debug, static_cache,
                                 verify_step=None if g == 1 else step, trace=trace)
