"""Autoregressive and beam-search decoding on the HIP path.

Drop-ins for sampling/base_decoding.py:9-187 (``autoregressive_generate``, ``beam_search_generate``):
same signatures, defaults and return values.  Model forwards stay in PyTorch-ROCm.

``autoregressive_generate`` draws each token with ``sd_sample`` (processor softmax + draw in one pass
over the row) straight into ``input_ids``; the host reads the token back once per step for the stop
test, as the reference's ``torch.isin`` branch does.  The model is called exactly as the reference
calls it — the whole prefix every step, with the cache object passed along under ``use_cache`` — so
the outputs equal the reference's whatever the model makes of that.

``beam_search_generate`` runs ONE ``sd_beam_step`` per step: log_softmax + topk of the beams' rows in
one pass, then the candidate loop, dedupe, stable sort and state update on the device, including the
reference's aliasing of a finished beam's score and last index (0-dim views).  The host reads one
word per step (``all_finished``).  Equal log-probs are ordered lowest index first, where
``torch.topk`` leaves the order undefined (beam step).
"""
from __future__ import annotations

from typing import List

import torch
from torch.nn import Module

from .. import _lib
from ..noise import default_noise, noise_session
from ..ops import BeamState, _user_process, beam_step, proc_spec, sample_rows
from ..utils.logits_processor import GreedyProcessor, LogitsProcessor


def _max_seq_length(model) -> int:
    cfg = model.config
    return cfg.max_position_embeddings if hasattr(cfg, "max_position_embeddings") else (
        cfg.max_context_length if hasattr(cfg, "max_context_length") else 1024)


def _require_gpu(model, what: str):
    dev = model.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError(f"specdec_amd.{what} runs on the GPU (HIP); the model is on {dev}. There is no CPU path.")
    return dev


@torch.no_grad()
def autoregressive_generate(
    inputs: List[int],
    model: Module,
    max_gen_len: int = 40,
    logits_processor: LogitsProcessor = GreedyProcessor(),
    eos_tokens_id: int | List[int] = 1,
    pad_token_id: int = 0,
    use_cache: bool = False,
    debug: bool = False,
) -> List[int]:
    """sampling/base_decoding.py:9-65."""
    noise = default_noise()
    with noise_session(noise):   # STREAM: the generator state stays on the device for the loop
        return _autoregressive_generate(noise, inputs, model, max_gen_len, logits_processor, eos_tokens_id,
                                        pad_token_id, use_cache, debug)


def _autoregressive_generate(noise, inputs, model, max_gen_len, logits_processor, eos_tokens_id, pad_token_id,
                             use_cache, debug):
    spec = proc_spec(logits_processor)   # a sample / __call__ override raises TypeError here
    kproc = logits_processor if _user_process(logits_processor) is not None else spec
    dev = _require_gpu(model, "autoregressive_generate")
    cache = None
    prompt_len = len(inputs)
    total_len = min(_max_seq_length(model), prompt_len + max_gen_len)                # :41-42
    input_ids = torch.full((1, total_len), pad_token_id, dtype=torch.long, device=dev)
    input_ids[0, :prompt_len] = torch.tensor(inputs, dtype=torch.long, device=dev)
    stops = eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    for curr in range(prompt_len, total_len):                                        # :51
        o = model(input_ids[..., :curr], past_key_values=cache, use_cache=use_cache)
        sample_rows(o.logits[..., -1, :], kproc, noise, tokens_out=input_ids[0, curr:curr + 1], status_or=err)
        cache = o.past_key_values
        x, bits = torch.stack([input_ids[0, curr], err[0].long()]).tolist()          # the step's one read
        _lib.raise_row_error(bits, "autoregressive_generate")
        if x in stops:                                                               # :60
            if debug:
                print(f"[specdec] end token found at position {curr}")
            break
    return input_ids[0, prompt_len:curr + 1].tolist()                                # :65


@torch.no_grad()
def beam_search_generate(
    inputs: List[int],
    model: Module,
    max_gen_len: int = 40,
    num_beams: int = 4,
    top_k: int = 3,
    min_length: float = 5.0,
    alpha: float = 1.2,
    eos_tokens_id: int | List[int] = 1,
    pad_token_id: int = 0,
    debug: bool = False,
    tokenizer=None,
) -> List[int]:
    """sampling/base_decoding.py:68-187."""
    dev = _require_gpu(model, "beam_search_generate")
    prompt_len = len(inputs)
    max_seq_length = _max_seq_length(model)
    assert prompt_len < max_seq_length, "Prompt length exceeds maximum sequence length."   # :112
    total_len = min(max_seq_length, prompt_len + max_gen_len)
    state = BeamState.start(inputs, num_beams, total_len, pad_token_id, dev)          # :115-125
    stops = torch.tensor(eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id], dtype=torch.long,
                         device=dev)
    kw = dict(alpha=alpha, min_length=min_length, stop_tokens=stops, pad_token_id=pad_token_id)

    o = model(state.input_ids[:, :prompt_len])                                       # :126
    # :127-131; writing position prompt_len of a row of total_len == prompt_len raises IndexError
    beam_step(state, o.logits[0:1, -1, :], prompt_len, prefill=True, length=1, **kw)
    for curr in range(prompt_len + 1, total_len):                                    # :133
        o = model(state.input_ids[:, :curr])
        done = beam_step(state, o.logits[:, -1, :], curr, top_k=top_k, length=curr - prompt_len, **kw)
        if debug:
            _print_beams(state, curr, tokenizer)
        done = int(done.item())                                                      # the step's one read
        if done < 0:   # the dedupe left fewer candidates than beams: possibilities[beam] (:175)
            raise IndexError("list index out of range")
        if done:                                                                     # :180
            if debug:
                print(f"[specdec] end token found at position {curr}")
            break
    last = int(state.last_indexes[0].item())                                         # :185-187
    if last == -1:
        last = total_len - 1
    return state.input_ids[0, prompt_len:last + 1].tolist()


def _print_beams(state: BeamState, curr: int, tokenizer) -> None:
    """debug=True: the step's beams, read back from the device."""
    ids, scores, last = state.input_ids.tolist(), state.beams_probs.tolist(), state.last_indexes.tolist()
    print(f"[specdec] beam step at position {curr}")
    for b, row in enumerate(ids):
        shown = tokenizer.decode(row[:curr + 1]) if tokenizer is not None else row[:curr + 1]
        print(f"  beam {b}: score {scores[b]:.6f} last {last[b]} {shown}")
