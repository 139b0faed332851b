"""Tensor-level wrappers over the C ABI (include/specdec.h).

Every call validates shapes, strides and dtypes on the host BEFORE a kernel is enqueued,
then launches on the current HIP stream of the tensors' device.  Nothing here syncs except
where noted: StreamNoise outside a ``session`` writes the moved generator state back to the
torch generator after each call (one device->host copy).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import lib
from .noise import PhiloxNoise, StreamNoise

_DT = {torch.float32: _lib.SD_F32, torch.bfloat16: _lib.SD_BF16, torch.float16: _lib.SD_F16}

KIND = {"greedy": _lib.SD_PROC_GREEDY, "multinomial": _lib.SD_PROC_MULTINOMIAL, "topk": _lib.SD_PROC_TOPK,
        "nucleus": _lib.SD_PROC_NUCLEUS, "topknucleus": _lib.SD_PROC_TOPK_NUCLEUS}
# the reference's class names (utils/logits_processor.py) and ours map to the same kinds
_CLASS_KIND = {"GreedyProcessor": "greedy", "MultinomialProcessor": "multinomial", "TopKProcessor": "topk",
               "NucleusProcessor": "nucleus", "TopKNucleusProcessor": "topknucleus"}


@dataclass(frozen=True)
class ProcSpec:
    kind: str = "greedy"
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0

    @property
    def stochastic(self) -> bool:
        return self.kind != "greedy"

    @property
    def keeps(self) -> bool:
        """top-k / nucleus: rows carry a keep predicate (sd_row_keep)"""
        return KIND[self.kind] >= _lib.SD_PROC_TOPK

    def struct(self) -> _lib.sd_processor:
        return _lib.sd_processor(KIND[self.kind], float(self.temperature), int(self.top_k), float(self.top_p))


PLAIN_SOFTMAX = ProcSpec("multinomial", 1.0)   # engine/infer_engine.py:241,276 (T=1, no processor)


# the processor protocol's behaviour (utils/logits_processor.py:7-23): a subclass that redefines the
# softmax or the sampling rule computes something the kernels do not, so it is refused, never run as
# its base class.  _process is the protocol's extension point: a subclass's own _process runs as it
# is (torch ops on the device rows) and the kernels take its output (_user_process).
_PROC_REFUSED = ("__call__", "sample")


def _known_base(proc):
    """(index in the MRO, name) of the first of the five processor classes proc derives from."""
    mro = type(proc).__mro__
    for i, cls in enumerate(mro):
        if cls.__name__ in _CLASS_KIND:
            return i, cls.__name__
    return -1, type(proc).__name__


def _user_process(proc):
    """The bound ``_process`` of a user subclass of one of the five processors that overrides it (the
    reference's extension point, utils/logits_processor.py:18-20), else None."""
    if isinstance(proc, ProcSpec):
        return None
    i, _ = _known_base(proc)
    if i <= 0:
        return None
    return proc._process if any("_process" in vars(sub) for sub in type(proc).__mro__[:i]) else None


def proc_spec(proc) -> ProcSpec:
    """ProcSpec of one of the five processors (ours, the reference's, or a ProcSpec).

    A subclass of a known processor may override ``_process`` (its own processing — often
    ``super()._process`` plus more): the rows are then processed by running it (``processed_rows``)
    and the kernels apply the base class's sampling rule to them — softmax(y / T), then argmax
    (GreedyProcessor) or the multinomial draw.  A subclass that overrides ``__call__`` or ``sample``
    raises TypeError: the kernels fuse the softmax and the draw and cannot run user code there."""
    if isinstance(proc, ProcSpec):
        return proc
    i, name = _known_base(proc)
    if i < 0:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}")
    mro = type(proc).__mro__
    for sub in mro[:i]:
        over = [m for m in _PROC_REFUSED if m in vars(sub)]
        if over:
            raise TypeError(f"unsupported logits processor {type(proc).__name__}: {sub.__name__} overrides "
                            f"{', '.join(over)} of {name}, which the fused kernels cannot run")
    T = float(getattr(proc, "temperature", 1.0))
    if _user_process(proc) is not None:   # user processing: only the base's sampling rule stays fused
        return ProcSpec("greedy" if name == "GreedyProcessor" else "multinomial", T)
    return ProcSpec(_CLASS_KIND[name], T, int(getattr(proc, "top_k", 0)), float(getattr(proc, "top_p", 1.0)))


def processed_rows(proc, rows):
    """The rows the kernels read for processor ``proc``: the rows themselves, or — for a subclass
    with its own ``_process`` — its output on a copy of each row (device torch ops; the caller's
    logits are never modified).  rows: a tensor [R, V] or a sequence of them."""
    fn = _user_process(proc)
    if fn is None:
        return rows

    def one(t):
        y = fn(t.clone())
        if not torch.is_tensor(y) or y.shape != t.shape or y.device != t.device:
            raise ValueError(f"{type(proc).__name__}._process must return a tensor of the input's shape and device")
        if y.dtype not in _DT:
            y = y.float()
        return y if y.stride(-1) == 1 else y.contiguous()

    return one(rows) if torch.is_tensor(rows) else [one(t) for t in rows]


# sequences one Philox call verifies / samples (the arrival-counter block, kCntMax in the kernels)
MAX_ROWS_PER_CALL = 16384


def _row_shards(B: int, noise):
    """Row shards of a Philox call over more than MAX_ROWS_PER_CALL sequences: [(r0, r1, noise)]
    with ONE call offset for all shards (noise keyed by the global row = row_base + r), so the
    shards draw what one call would.  None when the call fits (or is not Philox)."""
    if B <= MAX_ROWS_PER_CALL or not isinstance(noise, PhiloxNoise):
        return None
    o = noise.next_offset()
    return [(r0, min(B, r0 + MAX_ROWS_PER_CALL), PhiloxNoise(noise.seed, o, noise.offset_dev))
            for r0 in range(0, B, MAX_ROWS_PER_CALL)]


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# One workspace per (device, stream): it holds the arrival counters and partials of the calls in
# flight, so calls on different streams must not share one (they would mix their counters).  A
# workspace is allocated on the stream that uses it, so replacing it by a bigger one is
# stream-ordered by the caching allocator.  Graph capture reuses the device's largest eager
# workspace (the capture stream is a side stream; run the call eagerly once before capturing) and
# keeps it alive for as long as the process runs, since replays hold its address.
_WS: Dict[Tuple[torch.device, int], torch.Tensor] = {}
_GRAPH_WS: List[torch.Tensor] = []


def _workspace(nbytes: int, device) -> torch.Tensor:
    dev = torch.device(device)
    if torch.cuda.is_current_stream_capturing():
        cands = [w for (d, _), w in _WS.items() if d == dev]
        ws = max(cands, key=lambda w: w.numel()) if cands else None
        if ws is None or ws.numel() < nbytes:
            raise RuntimeError("specdec: a call captured into a hipGraph needs a workspace sized by an eager call "
                               "of the same shape first (run it once before capturing)")
        if not any(w is ws for w in _GRAPH_WS):
            _GRAPH_WS.append(ws)
        return ws
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        # zero-filled once: the library keeps its arrival counters (front of the workspace) at zero
        ws = torch.zeros(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _WS[key] = ws
    return ws


def _require_rows(t: torch.Tensor, name: str, V: int) -> None:
    if t.dim() != 2 or t.shape[1] != V:
        raise ValueError(f"{name}: expected [rows, {V}], got {tuple(t.shape)}")
    if t.stride(1) != 1:
        raise ValueError(f"{name}: vocab axis must be contiguous")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a device tensor")
    if t.dtype not in _DT:
        raise ValueError(f"{name}: unsupported dtype {t.dtype}")


def _status_or_ptr(status_or: Optional[torch.Tensor], device):
    """Device address of a caller's sticky error word (int32 [1] on the call's device), or None."""
    if status_or is None:
        return None
    if status_or.dtype != torch.int32 or status_or.numel() < 1 or status_or.device != torch.device(device):
        raise ValueError("status_or must be an int32 [1] tensor on the call's device")
    return status_or.data_ptr()


def _noise_struct(noise, n_words_needed: int, device, row_base: int = 0):
    """(sd_noise, keepalive tensor) for a call that may consume up to n_words_needed words.
    row_base: global id of the call's row 0 (Philox noise is keyed by the global row)."""
    if isinstance(noise, StreamNoise):
        # the call's words start at words[offset + *offset_dev] (ABI 11; a pipelined session's pool)
        words, off, off_dev = noise.prepare_ex(n_words_needed, device)
        return _lib.sd_noise(_lib.SD_NOISE_STREAM, words.data_ptr(), words.numel(), 0, int(off), 0,
                             off_dev.data_ptr() if off_dev is not None else None), (words, off_dev)
    if isinstance(noise, PhiloxNoise):
        if not 0 <= row_base < (1 << 24):
            raise ValueError("row_base must be in [0, 2^24)")
        od = noise.offset_dev
        if od is not None and (od.dtype != torch.int64 or od.numel() != 1 or od.device != torch.device(device)):
            raise ValueError("PhiloxNoise.offset_dev must be an int64 [1] tensor on the call's device")
        return _lib.sd_noise(_lib.SD_NOISE_PHILOX, None, 0, noise.seed, noise.next_offset(), row_base,
                             od.data_ptr() if od is not None else None), None
    raise TypeError(f"unsupported noise source {type(noise).__name__}")


# --------------------------------------------------------------------------- sampling
def sample_rows(logits: torch.Tensor, proc, noise, tokens_out: Optional[torch.Tensor] = None,
                want_prob: bool = False, row_base: int = 0, row_stats_out: Optional[torch.Tensor] = None,
                row_keep_out: Optional[torch.Tensor] = None, status_or: Optional[torch.Tensor] = None):
    """LogitsProcessor.__call__ + .sample on every row of logits [R, V] (one sample per row).

    Returns (tokens int64 [R], token_prob fp32 [R] or None, row_status int32 [R]).  Under
    StreamNoise the generator advances by 2·R·V words (torch.multinomial's Exp noise).
    row_stats_out: optional fp32 [R, 2] device tensor (contiguous) that receives each processed
    row's (max, Σexp) — what ``verify(draft_row_stats=...)`` takes so the verify step does not
    re-read the drafter rows.  Under PhiloxNoise stochastic rows are drawn in ONE pass (k_draw).
    row_keep_out: optional int32 [R, 4] contiguous device tensor that receives a top-k / nucleus
    row's keep predicate (sd_row_keep: tau as fp32 bits, tie index, flags) — what
    ``verify(draft_row_keep=...)`` takes with the stats so the verify skips the drafter rows'
    threshold search.  Not written for other processors.
    status_or: optional int32 [1] device word; every row's SD_ROW_ERROR_MASK bits are ORed into it
    (the decode loops test it where they already sync instead of reading every row_status).
    """
    spec = proc_spec(proc)
    R, V = logits.shape
    _require_rows(logits, "logits", V)
    logits = processed_rows(proc, logits)
    proc = spec
    dev = logits.device
    shards = _row_shards(R, noise)
    if shards is not None:   # more rows than one call holds: row shards, one noise offset
        toks = tokens_out if tokens_out is not None else torch.empty(R, dtype=torch.long, device=dev)
        outs = [sample_rows(logits[r0:r1], proc, nz, toks[r0:r1], want_prob, row_base + r0,
                            None if row_stats_out is None else row_stats_out.view(-1, 2)[r0:r1],
                            None if row_keep_out is None else row_keep_out.view(-1, 4)[r0:r1], status_or)
                for r0, r1, nz in shards]
        return (toks, torch.cat([o[1] for o in outs]) if want_prob else None, torch.cat([o[2] for o in outs]))
    tokens = tokens_out if tokens_out is not None else torch.empty(R, dtype=torch.long, device=dev)
    if tokens.dtype != torch.long or tokens.numel() < R or not tokens.is_cuda:
        raise ValueError("tokens_out must be an int64 device tensor with >= rows elements")
    prob = torch.empty(R, dtype=torch.float32, device=dev) if want_prob else None
    status = torch.empty(R, dtype=torch.int32, device=dev)
    if row_stats_out is not None and (row_stats_out.dtype != torch.float32 or not row_stats_out.is_cuda
                                      or row_stats_out.numel() < 2 * R or not row_stats_out.is_contiguous()):
        raise ValueError("row_stats_out must be a contiguous fp32 device tensor with >= 2*rows elements")
    if row_keep_out is not None and (row_keep_out.dtype != torch.int32 or not row_keep_out.is_cuda
                                     or row_keep_out.numel() < 4 * R or not row_keep_out.is_contiguous()):
        raise ValueError("row_keep_out must be a contiguous int32 device tensor with >= 4*rows elements")
    need = 2 * R * V if spec.stochastic else 0
    nz, keep = _noise_struct(noise, need, dev, row_base)
    nbytes = lib.sd_sample_workspace_size(R, V)
    ws = _workspace(nbytes, dev)
    a = _lib.sd_sample_args(R, V, logits.data_ptr(), logits.stride(0), _DT[logits.dtype], spec.struct(), nz,
                            tokens.data_ptr(), tokens.stride(0) if tokens.dim() == 1 else 1,
                            prob.data_ptr() if prob is not None else None, status.data_ptr(), None,
                            ws.data_ptr(), ws.numel(),
                            row_stats_out.data_ptr() if row_stats_out is not None else None,
                            row_keep_out.data_ptr() if row_keep_out is not None else None,
                            _status_or_ptr(status_or, dev))
    _lib.check(lib.sd_sample(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_sample")
    if isinstance(noise, StreamNoise):
        noise.consumed(count=need)
    del keep
    return tokens, prob, status


def probs_rows(logits: torch.Tensor, proc) -> torch.Tensor:
    """LogitsProcessor.__call__: softmax(_process(logits) / T) in the logits dtype, on the device."""
    spec = proc_spec(proc)
    shape = logits.shape
    x = processed_rows(proc, logits.reshape(-1, shape[-1]))
    if x.stride(-1) != 1:
        x = x.contiguous()
    R, V = x.shape
    _require_rows(x, "logits", V)
    out = torch.empty((R, V), dtype=x.dtype, device=x.device)
    ws = _workspace(lib.sd_probs_workspace_size(R, V), x.device)
    a = _lib.sd_probs_args(R, V, x.data_ptr(), x.stride(0), _DT[x.dtype], spec.struct(), out.data_ptr(),
                           out.stride(0), ws.data_ptr(), ws.numel())
    _lib.check(lib.sd_probs(C.byref(a), C.c_void_p(_stream_ptr(x.device))), "sd_probs")
    return out.reshape(shape)


# --------------------------------------------------------------------------- verify
@dataclass
class VerifyOut:
    n_accepted: torch.Tensor      # int32 [B]
    next_token: torch.Tensor      # int64 [B]
    resample_mass: torch.Tensor   # fp32  [B]
    prune_drafter: torch.Tensor   # int32 [B]
    prune_target: torch.Tensor    # int32 [B]
    stop_index: torch.Tensor      # int32 [B]
    row_status: torch.Tensor      # int32 [B]
    words_used: torch.Tensor      # int64 [1]


def _verify_outputs(B: int, dev) -> VerifyOut:
    """VerifyOut's eight tensors as views of one device buffer: int64 fields first (8-byte aligned),
    then the 4-byte ones."""
    buf = torch.empty(8 * (B + 1) + 4 * 6 * B, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    used = buf[8 * B:8 * (B + 1)].view(torch.long)
    f4 = buf[8 * (B + 1):].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(6)]
    return VerifyOut(i32[0], nxt, i32[1].view(torch.float32), i32[2], i32[3], i32[4], i32[5], used)


def verify(target_rows: Sequence[torch.Tensor], draft_rows: Sequence[torch.Tensor], draft_tokens: torch.Tensor,
           rule: int, target_proc, draft_proc, noise, stop_tokens: Optional[torch.Tensor] = None,
           skip_sample_adjustment: bool = False, draft_is_probs: bool = False,
           active: Optional[torch.Tensor] = None, engine_state: Optional[dict] = None,
           sync_noise: bool = True, prof_events=None, row_base: int = 0,
           draft_row_stats: Optional[torch.Tensor] = None,
           draft_row_keep: Optional[torch.Tensor] = None,
           status_or: Optional[torch.Tensor] = None,
           row_counts: Optional[torch.Tensor] = None) -> VerifyOut:
    """One verify step for B sequences.

    target_rows: γ+1 (SPEC) or γ (ENGINE) tensors [B, V] — row t of every sequence;
    draft_rows:  γ tensors [B, V] (logits, or fp32 probabilities with draft_is_probs);
    draft_tokens: int64 [B, >=γ].  Under StreamNoise the torch generator is advanced by the
    words the kernels consumed, which needs one device->host read (sync_noise).
    row_base: global row id of this call's row 0 under PhiloxNoise (data-parallel shards draw
    what one call over the whole batch would draw for the same rows).
    draft_row_stats: optional fp32 [γ, B, 2] (or [γ, S>=B, 2]) device tensor — the drafter rows'
    (max, Σexp) as ``sample_rows(row_stats_out=...)`` returned them with the draws; the
    row-statistics pass then reads only the target rows.  Ignored for a top-k / nucleus drafter
    unless draft_row_keep comes with it.
    draft_row_keep: optional int32 [γ, S, 4] device tensor at draft_row_stats' row layout — the
    drafter rows' keep predicates as ``sample_rows(row_keep_out=...)`` returned them; the
    threshold search then covers the target rows only.
    status_or: optional int32 [1] device word that collects every row's SD_ROW_ERROR_MASK bits.
    row_counts: optional int64 [B, 2] contiguous device tensor; each call ADDS (accepted drafts,
    tokens emitted) to every row's pair (the A12 bookkeeping, kept on the device).
    """
    gamma = len(draft_rows)
    if rule == _lib.SD_RULE_SPEC and (active is not None or engine_state is not None):
        # the batch-1 rule has no finished rows and no engine state (sampling/speculative_decoding.py:
        # 129-171); refused on every path, so a γ > SD_MAX_GAMMA window cannot drop them silently
        raise ValueError("active / engine_state belong to the ENGINE rule (SD_RULE_ENGINE)")
    # user _process overrides: the kernels read the processed rows (processed_rows)
    target_rows = processed_rows(target_proc, list(target_rows))
    if not draft_is_probs:
        draft_rows = processed_rows(draft_proc, list(draft_rows))
    target_proc, draft_proc = proc_spec(target_proc), proc_spec(draft_proc)
    if gamma > _lib.SD_MAX_GAMMA:   # the reference takes any γ: windows of <= SD_MAX_GAMMA drafts (chunked.py)
        if prof_events is not None:
            raise ValueError("prof_events needs gamma <= SD_MAX_GAMMA")
        from .chunked import verify_chunked
        return verify_chunked(target_rows, draft_rows, draft_tokens, rule, target_proc, draft_proc, noise,
                              stop_tokens, skip_sample_adjustment, draft_is_probs, active, engine_state, sync_noise,
                              row_base, draft_row_stats, draft_row_keep, status_or, row_counts)
    if not 1 <= gamma:
        raise ValueError(f"gamma must be >= 1, got {gamma}")
    n_t = gamma + 1 if rule == _lib.SD_RULE_SPEC else gamma
    if len(target_rows) != n_t:
        raise ValueError(f"expected {n_t} target rows, got {len(target_rows)}")
    B, V = target_rows[0].shape
    dev = target_rows[0].device
    shards = _row_shards(B, noise)
    if shards is not None:   # more sequences than one call holds: row shards, one noise offset
        outs = []
        for r0, r1, nz in shards:
            es = None
            if engine_state is not None:
                es = dict(generated=engine_state["generated"][r0:r1], step=engine_state["step"],
                          finished=engine_state["finished"][r0:r1], accepted=engine_state["accepted"][r0:r1])
            outs.append(verify([t[r0:r1] for t in target_rows], [d[r0:r1] for d in draft_rows], draft_tokens[r0:r1],
                               rule, target_proc, draft_proc, nz, stop_tokens, skip_sample_adjustment, draft_is_probs,
                               None if active is None else active[r0:r1], es, sync_noise, None, row_base + r0,
                               None if draft_row_stats is None else draft_row_stats[:, r0:r1],
                               None if draft_row_keep is None else draft_row_keep[:, r0:r1], status_or,
                               None if row_counts is None else row_counts[r0:r1]))
        cat = {f: torch.cat([getattr(o, f) for o in outs]) for f in VerifyOut.__dataclass_fields__ if f != "words_used"}
        return VerifyOut(**cat, words_used=torch.zeros(1, dtype=torch.long, device=dev))
    tdt = target_rows[0].dtype
    # the batch stride is shared by a row set (it is irrelevant when B == 1)
    t_stride = target_rows[0].stride(0) if B > 1 else 0
    d_stride = draft_rows[0].stride(0) if B > 1 else 0
    for i, t in enumerate(target_rows):
        _require_rows(t, f"target_rows[{i}]", V)
        if t.shape[0] != B or t.dtype != tdt or (B > 1 and t.stride(0) != t_stride) or t.device != dev:
            raise ValueError("target rows must share batch, dtype, batch stride and device")
    for i, d in enumerate(draft_rows):
        _require_rows(d, f"draft_rows[{i}]", V)
        if d.shape[0] != B or d.dtype != draft_rows[0].dtype or (B > 1 and d.stride(0) != d_stride) \
                or d.device != dev:
            raise ValueError("draft rows must share batch, dtype, batch stride and device")
    if draft_is_probs and draft_rows[0].dtype != torch.float32:
        raise ValueError("draft probabilities must be fp32")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != B \
            or draft_tokens.shape[1] < gamma or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B, >={gamma}] on {dev}")
    tspec, dspec = proc_spec(target_proc), proc_spec(draft_proc)
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev:
        raise ValueError("stop_tokens must be an int64 device tensor")
    if active is not None and (active.dtype not in (torch.uint8, torch.bool) or active.numel() != B):
        raise ValueError("active must be uint8/bool [B]")
    if draft_row_stats is not None:
        ds = draft_row_stats
        if ds.dtype != torch.float32 or ds.dim() != 3 or ds.shape[0] < gamma or ds.shape[1] < B \
                or ds.shape[2] != 2 or ds.stride(2) != 1 or ds.stride(1) != 2 or ds.device != dev:
            raise ValueError(f"draft_row_stats must be fp32 [>={gamma}, >={B}, 2] with (max, sum) pairs on {dev}")
    if draft_row_keep is not None:
        dk = draft_row_keep
        if draft_row_stats is None or dk.dtype != torch.int32 or dk.dim() != 3 or dk.shape[0] < gamma \
                or dk.shape[1] < B or dk.shape[2] != 4 or dk.stride(2) != 1 or dk.stride(1) != 4 \
                or dk.stride(0) // 4 != draft_row_stats.stride(0) // 2 or dk.device != dev:
            raise ValueError("draft_row_keep must be int32 [>=gamma, >=B, 4] at draft_row_stats' row stride, "
                             "and comes with draft_row_stats")

    # every output is written by the kernels (no fill launches); one allocation, typed views of it
    # (eight caching-allocator calls per verify were a visible share of an eager step's host time)
    out = _verify_outputs(B, dev)
    stochastic = rule == _lib.SD_RULE_ENGINE or tspec.stochastic
    need = B * (gamma + (2 * V if stochastic else 0))
    nz, keep = _noise_struct(noise, need, dev, row_base)
    ws = _workspace(lib.sd_verify_workspace_size(B, gamma, V), dev)

    a = _lib.sd_verify_args()
    a.batch, a.gamma, a.vocab, a.rule = B, gamma, V, rule
    for i, t in enumerate(target_rows):
        a.target_rows[i] = t.data_ptr()
    a.target_stride_b, a.target_dtype = t_stride, _DT[tdt]
    for i, d in enumerate(draft_rows):
        a.draft_rows[i] = d.data_ptr()
    a.draft_stride_b, a.draft_dtype = d_stride, _DT[draft_rows[0].dtype]
    a.draft_is_probs = int(draft_is_probs)
    a.draft_tokens, a.draft_tokens_stride_b = draft_tokens.data_ptr(), draft_tokens.stride(0)
    a.target_proc, a.draft_proc = tspec.struct(), dspec.struct()
    a.skip_sample_adjustment = int(skip_sample_adjustment)
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.active = active.data_ptr() if active is not None else None
    a.noise = nz
    a.n_accepted, a.next_token, a.resample_mass = out.n_accepted.data_ptr(), out.next_token.data_ptr(), \
        out.resample_mass.data_ptr()
    a.prune_drafter, a.prune_target = out.prune_drafter.data_ptr(), out.prune_target.data_ptr()
    a.stop_index, a.row_status, a.words_used = out.stop_index.data_ptr(), out.row_status.data_ptr(), \
        out.words_used.data_ptr()
    if engine_state is not None:
        gen, fin, acc = engine_state["generated"], engine_state["finished"], engine_state["accepted"]
        if gen.dtype != torch.long or gen.shape[0] != B or gen.stride(1) != 1:
            raise ValueError("engine generated must be int64 [B, gen_len]")
        if engine_state["step"] + gamma > gen.shape[1]:
            raise ValueError("engine step window exceeds generated length")
        if fin.dtype not in (torch.uint8, torch.bool) or acc.dtype != torch.long:
            raise ValueError("engine finished must be uint8/bool, accepted int64")
        a.generated, a.generated_stride_b, a.step = gen.data_ptr(), gen.stride(0), int(engine_state["step"])
        a.finished, a.accepted_count = fin.data_ptr(), acc.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if draft_row_stats is not None:
        a.draft_row_stats, a.draft_row_stats_stride = draft_row_stats.data_ptr(), draft_row_stats.stride(0) // 2
    if draft_row_keep is not None:
        a.draft_row_keep = draft_row_keep.data_ptr()
    a.status_or = _status_or_ptr(status_or, dev)
    if row_counts is not None:
        if row_counts.dtype != torch.long or tuple(row_counts.shape) != (B, 2) or not row_counts.is_contiguous() \
                or row_counts.device != dev:
            raise ValueError(f"row_counts must be a contiguous int64 [{B}, 2] tensor on {dev}")
        a.row_counts = row_counts.data_ptr()
    if prof_events is not None:   # (torch.cuda.Event, torch.cuda.Event[, repeats]) around the row-stats kernel
        a.prof_stats_begin, a.prof_stats_end = prof_events[0].cuda_event, prof_events[1].cuda_event
        a.prof_stats_repeat = int(prof_events[2]) if len(prof_events) > 2 else 1
    _lib.check(lib.sd_verify(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify")
    if isinstance(noise, StreamNoise) and sync_noise:
        noise.consumed(used_dev=out.words_used)
    del keep
    return out


# --------------------------------------------------------------------------- multi-draft verify
MULTI_FIELDS = ("n_accepted", "winner", "next_token", "resample_mass", "n_sibling_rejects", "prune_drafter",
                "prune_target", "stop_index", "row_status")


def _chain_rows(x, name: str, n_rows: int):
    """Per-depth row tensors [B*K, V] of a [B, K, n_rows, V] tensor (views), or the sequence given."""
    if torch.is_tensor(x):
        if x.dim() != 4 or x.shape[2] != n_rows:
            raise ValueError(f"{name}: expected [B, K, {n_rows}, V], got {tuple(x.shape)}")
        B, K, _, V = x.shape
        if B > 1 and x.stride(0) != K * x.stride(1):
            x = x.contiguous()
        return [x[:, :, t, :].as_strided((B * K, V), (x.stride(1), x.stride(3)), x[:, :, t, :].storage_offset())
                for t in range(n_rows)]
    return list(x)


def verify_multi(target, draft, draft_tokens: torch.Tensor, proc, noise, num_drafts: Optional[int] = None,
                 stop_tokens: Optional[torch.Tensor] = None, row_base: int = 0,
                 draft_row_stats: Optional[torch.Tensor] = None, draft_row_keep: Optional[torch.Tensor] = None,
                 status_or: Optional[torch.Tensor] = None, pad_token_id: int = 0, want_tokens: bool = True):
    """One multi-draft verify step (sd_verify_multi): K independently drafted chains of γ tokens per
    sequence, walked as a prefix tree by recursive rejection sampling, so the emitted tokens keep the
    target's distribution exactly.

    target: [B, K, γ+1, V] logits (or γ+1 tensors [B*K, V], chain k of sequence b at row b*K + k);
    draft: [B, K, γ, V] (or γ tensors [B*K, V]); draft_tokens: int64 [B, K, >=γ] or [B*K, >=γ].
    proc: one of the five processors, used for target and drafter rows alike.  noise: PhiloxNoise
    (one offset per call).  draft_row_stats fp32 [γ, S>=B*K, 2] / draft_row_keep int32 [γ, S, 4]: the
    drafter rows' statistics as ``sample_rows`` returned them with the draws (hints, as ``verify``'s).
    Returns a namespace of the [B] outputs n_accepted, winner, next_token, resample_mass,
    n_sibling_rejects, prune_drafter, prune_target, stop_index, row_status, and tokens_out int64
    [B, γ+1] (tok[winner, :n], then x, then pad_token_id; None without want_tokens)."""
    from types import SimpleNamespace
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: verify_multi fuses the processing "
                        "of target and drafter rows and cannot run a user _process")
    spec = proc_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_multi needs PhiloxNoise (the reference defines no stream order for this step)")
    if torch.is_tensor(target) and num_drafts is None:
        num_drafts = target.shape[1]
    K = int(num_drafts) if num_drafts is not None else (draft_tokens.shape[1] if draft_tokens.dim() == 3 else 0)
    if draft_tokens.dim() == 3:
        if draft_tokens.shape[1] != K:
            raise ValueError(f"draft_tokens: expected [B, {K}, >=gamma], got {tuple(draft_tokens.shape)}")
        draft_tokens = draft_tokens.reshape(-1, draft_tokens.shape[-1])
    draft_rows = _chain_rows(draft, "draft", draft.shape[2] if torch.is_tensor(draft) else len(draft))
    gamma = len(draft_rows)
    target_rows = _chain_rows(target, "target", gamma + 1)
    if len(target_rows) != gamma + 1:
        raise ValueError(f"expected {gamma + 1} target rows, got {len(target_rows)}")
    R, V = target_rows[0].shape
    if not 1 <= K <= _lib.SD_MULTI_MAX_DRAFTS or R % K or not 1 <= gamma <= _lib.SD_MAX_GAMMA \
            or K * gamma > _lib.SD_MULTI_MAX_NODES or R > _lib.SD_MULTI_MAX_ROWS:
        raise ValueError(f"verify_multi: unsupported shape (rows {R}, num_drafts {K}, gamma {gamma}): K in 1..8, "
                         f"gamma in 1..{_lib.SD_MAX_GAMMA}, K * gamma <= 64, B * K <= 16384")
    B = R // K
    dev, tdt = target_rows[0].device, target_rows[0].dtype
    t_stride = target_rows[0].stride(0) if R > 1 else 0
    d_stride = draft_rows[0].stride(0) if R > 1 else 0
    for name, rows, stride in (("target", target_rows, t_stride), ("draft", draft_rows, d_stride)):
        for i, t in enumerate(rows):
            _require_rows(t, f"{name}_rows[{i}]", V)
            if t.shape[0] != R or t.dtype != tdt or (R > 1 and t.stride(0) != stride) or t.device != dev:
                raise ValueError("target and draft rows must share rows, dtype, row stride and device")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != R \
            or draft_tokens.shape[1] < gamma or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B*K, >={gamma}] on {dev}")
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 device tensor")
    if draft_row_stats is not None:
        ds = draft_row_stats
        if ds.dtype != torch.float32 or ds.dim() != 3 or ds.shape[0] < gamma or ds.shape[1] < R \
                or ds.shape[2] != 2 or ds.stride(2) != 1 or ds.stride(1) != 2 or ds.device != dev:
            raise ValueError(f"draft_row_stats must be fp32 [>={gamma}, >={R}, 2] with (max, sum) pairs on {dev}")
    if draft_row_keep is not None:
        dk = draft_row_keep
        if draft_row_stats is None or dk.dtype != torch.int32 or dk.dim() != 3 or dk.shape[0] < gamma \
                or dk.shape[1] < R or dk.shape[2] != 4 or dk.stride(2) != 1 or dk.stride(1) != 4 \
                or dk.stride(0) // 4 != draft_row_stats.stride(0) // 2 or dk.device != dev:
            raise ValueError("draft_row_keep must be int32 [>=gamma, >=B*K, 4] at draft_row_stats' row stride, "
                             "and comes with draft_row_stats")
    # one allocation: next_token (int64) first, then the eight 4-byte fields
    buf = torch.empty(8 * B + 4 * 8 * B, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    f4 = buf[8 * B:].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(8)]
    out = SimpleNamespace(n_accepted=i32[0], winner=i32[1], next_token=nxt, resample_mass=i32[2].view(torch.float32),
                          n_sibling_rejects=i32[3], prune_drafter=i32[4], prune_target=i32[5], stop_index=i32[6],
                          row_status=i32[7],
                          tokens_out=torch.empty(B, gamma + 1, dtype=torch.long, device=dev) if want_tokens else None)
    nz, keep = _noise_struct(noise, 0, dev, row_base)
    ws = _workspace(lib.sd_verify_multi_workspace_size(B, K, gamma, V), dev)
    a = _lib.sd_multi_args()
    a.batch, a.num_drafts, a.gamma, a.vocab = B, K, gamma, V
    for i, t in enumerate(target_rows):
        a.target_rows[i] = t.data_ptr()
    for i, d in enumerate(draft_rows):
        a.draft_rows[i] = d.data_ptr()
    a.target_stride_r, a.draft_stride_r = t_stride, d_stride
    a.target_dtype = a.draft_dtype = _DT[tdt]
    a.draft_tokens, a.draft_tokens_stride_r = draft_tokens.data_ptr(), draft_tokens.stride(0)
    a.proc = spec.struct()
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.pad_token = int(pad_token_id)
    a.noise = nz
    for f in MULTI_FIELDS:
        setattr(a, f, getattr(out, f).data_ptr())
    if want_tokens:
        a.tokens_out, a.tokens_out_stride_b = out.tokens_out.data_ptr(), gamma + 1
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if draft_row_stats is not None:
        a.draft_row_stats, a.draft_row_stats_stride = draft_row_stats.data_ptr(), draft_row_stats.stride(0) // 2
    if draft_row_keep is not None:
        a.draft_row_keep = draft_row_keep.data_ptr()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_verify_multi(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify_multi")
    del keep
    return out


# --------------------------------------------------------------------------- block verify
BLOCK_FIELDS = ("n_accepted", "next_token", "resample_mass", "prune_drafter", "prune_target", "stop_index",
                "row_status")


@dataclass
class BlockVerifyOut:
    """``VerifyOut``'s per-sequence outputs of one block verify step, plus the rule's diagnostics:
    weights fp32 [B, γ+1] (w_0..w_γ) and accept_prob fp32 [B, γ] (h_1..h_γ); tokens_out int64
    [B, γ+1] (tok[:n], then x, then pad_token_id; None without want_tokens)."""
    n_accepted: torch.Tensor
    next_token: torch.Tensor
    resample_mass: torch.Tensor
    prune_drafter: torch.Tensor
    prune_target: torch.Tensor
    stop_index: torch.Tensor
    row_status: torch.Tensor
    weights: torch.Tensor
    accept_prob: torch.Tensor
    tokens_out: Optional[torch.Tensor] = None


def verify_block(target, draft, draft_tokens: torch.Tensor, proc, noise,
                 stop_tokens: Optional[torch.Tensor] = None, row_base: int = 0,
                 draft_row_stats: Optional[torch.Tensor] = None, draft_row_keep: Optional[torch.Tensor] = None,
                 status_or: Optional[torch.Tensor] = None, pad_token_id: int = 0, want_tokens: bool = True):
    """One block verify step (sd_verify_block): the γ drafted tokens of one chain per sequence are
    verified jointly (block verification), which is lossless and accepts at least as many tokens in
    expectation as ``verify``'s token-wise SD_RULE_SPEC test on the same rows and drafts.

    target: [B, γ+1, V] logits (or γ+1 tensors [B, V]); draft: [B, γ, V] (or γ tensors [B, V]);
    draft_tokens: int64 [B, >=γ].  proc: one of the five processors, used for target and drafter rows
    alike.  noise: PhiloxNoise (one offset per call).  draft_row_stats fp32 [γ, S>=B, 2] /
    draft_row_keep int32 [γ, S, 4]: the drafter rows' statistics as ``sample_rows`` returned them with
    the draws (hints, as ``verify``'s).  Returns a BlockVerifyOut."""
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: verify_block fuses the processing "
                        "of target and drafter rows and cannot run a user _process")
    spec = proc_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_block needs PhiloxNoise (the rule defines no stream order)")
    draft_rows = [draft[:, t, :] for t in range(draft.shape[1])] if torch.is_tensor(draft) else list(draft)
    gamma = len(draft_rows)
    target_rows = [target[:, t, :] for t in range(target.shape[1])] if torch.is_tensor(target) else list(target)
    if len(target_rows) != gamma + 1:
        raise ValueError(f"expected {gamma + 1} target rows, got {len(target_rows)}")
    B, V = target_rows[0].shape
    if not 1 <= gamma <= _lib.SD_MAX_GAMMA or not 1 <= B <= _lib.SD_MULTI_MAX_ROWS:
        raise ValueError(f"verify_block: unsupported shape (batch {B}, gamma {gamma}): gamma in "
                         f"1..{_lib.SD_MAX_GAMMA}, batch in 1..{_lib.SD_MULTI_MAX_ROWS}")
    dev, tdt = target_rows[0].device, target_rows[0].dtype
    t_stride = target_rows[0].stride(0) if B > 1 else 0
    d_stride = draft_rows[0].stride(0) if B > 1 else 0
    for name, rows, stride in (("target", target_rows, t_stride), ("draft", draft_rows, d_stride)):
        for i, t in enumerate(rows):
            _require_rows(t, f"{name}_rows[{i}]", V)
            if t.shape[0] != B or t.dtype != tdt or (B > 1 and t.stride(0) != stride) or t.device != dev:
                raise ValueError("target and draft rows must share batch, dtype, row stride and device")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != B \
            or draft_tokens.shape[1] < gamma or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B, >={gamma}] on {dev}")
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 device tensor")
    if draft_row_stats is not None:
        ds = draft_row_stats
        if ds.dtype != torch.float32 or ds.dim() != 3 or ds.shape[0] < gamma or ds.shape[1] < B \
                or ds.shape[2] != 2 or ds.stride(2) != 1 or ds.stride(1) != 2 or ds.device != dev:
            raise ValueError(f"draft_row_stats must be fp32 [>={gamma}, >={B}, 2] with (max, sum) pairs on {dev}")
    if draft_row_keep is not None:
        dk = draft_row_keep
        if draft_row_stats is None or dk.dtype != torch.int32 or dk.dim() != 3 or dk.shape[0] < gamma \
                or dk.shape[1] < B or dk.shape[2] != 4 or dk.stride(2) != 1 or dk.stride(1) != 4 \
                or dk.stride(0) // 4 != draft_row_stats.stride(0) // 2 or dk.device != dev:
            raise ValueError("draft_row_keep must be int32 [>=gamma, >=B, 4] at draft_row_stats' row stride, "
                             "and comes with draft_row_stats")
    # one allocation: next_token (int64) first, then the six 4-byte fields and the two diagnostics
    n4 = 6 * B + B * (gamma + 1) + B * gamma
    buf = torch.empty(8 * B + 4 * n4, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    f4 = buf[8 * B:].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(6)]
    wts = f4[6 * B:6 * B + B * (gamma + 1)].view(torch.float32).view(B, gamma + 1)
    acc = f4[6 * B + B * (gamma + 1):].view(torch.float32).view(B, gamma)
    out = BlockVerifyOut(n_accepted=i32[0], next_token=nxt, resample_mass=i32[1].view(torch.float32),
                         prune_drafter=i32[2], prune_target=i32[3], stop_index=i32[4], row_status=i32[5],
                         weights=wts, accept_prob=acc,
                         tokens_out=torch.empty(B, gamma + 1, dtype=torch.long, device=dev) if want_tokens else None)
    nz, keep = _noise_struct(noise, 0, dev, row_base)
    ws = _workspace(lib.sd_verify_block_workspace_size(B, gamma, V), dev)
    a = _lib.sd_block_args()
    a.batch, a.gamma, a.vocab = B, gamma, V
    for i, t in enumerate(target_rows):
        a.target_rows[i] = t.data_ptr()
    for i, d in enumerate(draft_rows):
        a.draft_rows[i] = d.data_ptr()
    a.target_stride_b, a.draft_stride_b = t_stride, d_stride
    a.target_dtype = a.draft_dtype = _DT[tdt]
    a.draft_tokens, a.draft_tokens_stride_b = draft_tokens.data_ptr(), max(draft_tokens.stride(0), gamma)
    a.proc = spec.struct()
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.pad_token = int(pad_token_id)
    a.noise = nz
    for f in BLOCK_FIELDS + ("weights", "accept_prob"):
        setattr(a, f, getattr(out, f).data_ptr())
    if want_tokens:
        a.tokens_out, a.tokens_out_stride_b = out.tokens_out.data_ptr(), gamma + 1
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if draft_row_stats is not None:
        a.draft_row_stats, a.draft_row_stats_stride = draft_row_stats.data_ptr(), draft_row_stats.stride(0) // 2
    if draft_row_keep is not None:
        a.draft_row_keep = draft_row_keep.data_ptr()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_verify_block(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify_block")
    del keep
    return out


# --------------------------------------------------------------------------- token-tree verify
TREE_FIELDS = ("n_accepted", "last_node", "next_token", "resample_mass", "n_sibling_rejects", "stop_index",
               "row_status")


def _tree_of(parent):
    from .tree import TokenTree
    return parent if isinstance(parent, TokenTree) else TokenTree(parent)


_ROW_PTRS = C.c_void_p * (_lib.SD_TREE_MAX_NODES + 1)


def _slot_rows(x, name: str, slots, n_slots: int, like):
    """(addresses by slot (None where the slot is not in `slots`), batch stride, B, V, dtype, device)
    of the rows of `slots`: x is a tensor [B, len(slots), V] holding them in order, or a sequence of
    n_slots entries [B, V] (entries outside `slots` are ignored).  like: the (B, V, dtype, device) the
    rows must share with the other side, or None."""
    ptrs = [None] * n_slots
    if torch.is_tensor(x):
        if x.dim() != 3 or x.shape[1] != len(slots):
            raise ValueError(f"{name}: expected [B, {len(slots)}, V], got {tuple(x.shape)}")
        B, _, V = x.shape
        _require_rows(x[:, 0, :], f"{name}_rows", V)
        step = x.stride(1) * x.element_size()
        base = x.data_ptr()
        for i, s in enumerate(slots):
            ptrs[s] = base + i * step
        stride, dt, dev = (x.stride(0) if B > 1 else 0), x.dtype, x.device
    else:
        rows = list(x)
        if len(rows) != n_slots:
            raise ValueError(f"expected {n_slots} {name} entries, got {len(rows)}")
        first = rows[slots[0]]
        if first is None:
            raise ValueError(f"{name}_rows[{slots[0]}]: slot {slots[0]} needs a row")
        B, V = first.shape[0], first.shape[-1]
        stride, dt, dev = (first.stride(0) if B > 1 else 0), first.dtype, first.device
        for s in slots:
            t = rows[s]
            if t is None:
                raise ValueError(f"{name}_rows[{s}]: slot {s} has children and needs a drafter row")
            _require_rows(t, f"{name}_rows[{s}]", V)
            if t.shape[0] != B or t.dtype != dt or (B > 1 and t.stride(0) != stride) or t.device != dev:
                raise ValueError(f"{name} rows must share batch, dtype, row stride and device")
            ptrs[s] = t.data_ptr()
    if like is not None and (B, V, dt, dev) != like:
        raise ValueError("target and draft rows must share batch, vocabulary, dtype and device")
    return ptrs, stride, B, V, dt, dev


def verify_tree(target, draft, draft_tokens: torch.Tensor, parent, proc, noise,
                stop_tokens: Optional[torch.Tensor] = None, row_base: int = 0,
                status_or: Optional[torch.Tensor] = None, pad_token_id: int = 0, want_tokens: bool = True):
    """One token-tree verify step (sd_verify_tree): N drafted nodes per sequence with parents
    ``parent`` (a TokenTree or a parent list; one topology for the whole call), walked from the root by
    recursive rejection sampling, so the emitted tokens keep the target's distribution exactly.

    target: [B, N+1, V] logits (or N+1 tensors [B, V]): slot 0 the root's row, slot i+1 the row after
    node i.  draft: a list of N+1 entries [B, V] with None at leaf slots, or a [B, I, V] tensor holding
    the internal slots' rows in ascending slot order.  draft_tokens: int64 [B, >=N].  proc: one of the
    five processors, used for target and drafter rows alike.  noise: PhiloxNoise (one offset per call).
    Returns a namespace of the [B] outputs n_accepted, last_node, next_token, resample_mass,
    n_sibling_rejects, stop_index, row_status, of path int32 [B, depth] (the node accepted at each
    depth, -1 beyond n) and tokens_out int64 [B, depth+1] (the path's tokens, then x, then
    pad_token_id; None without want_tokens)."""
    from types import SimpleNamespace
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: verify_tree fuses the processing "
                        "of target and drafter rows and cannot run a user _process")
    spec = proc_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_tree needs PhiloxNoise (the rule defines no stream order for this step)")
    tree = _tree_of(parent)
    N, depth = tree.num_nodes, tree.depth
    internal = tree.internal_slots
    # slot -> device address of its row of sequence 0, and the batch stride in elements
    t_ptrs, t_stride, B, V, tdt, dev = _slot_rows(target, "target", list(range(N + 1)), N + 1, None)
    d_ptrs, d_stride, _, _, _, _ = _slot_rows(draft, "draft", internal, N + 1, (B, V, tdt, dev))
    if not 1 <= B <= _lib.SD_TREE_MAX_BATCH:
        raise ValueError(f"verify_tree: batch must be in 1..{_lib.SD_TREE_MAX_BATCH}, got {B}")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != B \
            or draft_tokens.shape[1] < N or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B, >={N}] on {dev}")
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 device tensor")
    # one allocation: next_token (int64) first, then the six 4-byte fields and the path
    buf = torch.empty(8 * B + 4 * (6 + depth) * B, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    f4 = buf[8 * B:].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(6)]
    out = SimpleNamespace(n_accepted=i32[0], last_node=i32[1], next_token=nxt, resample_mass=i32[2].view(torch.float32),
                          n_sibling_rejects=i32[3], stop_index=i32[4], row_status=i32[5],
                          path=f4[6 * B:].view(B, depth),
                          tokens_out=torch.empty(B, depth + 1, dtype=torch.long, device=dev) if want_tokens else None)
    nz, keep = _noise_struct(noise, 0, dev, row_base)
    par = getattr(tree, "_c_parent", None)
    if par is None:
        par = tree._c_parent = (C.c_int32 * _lib.SD_TREE_MAX_NODES)(*tree.parent)
    ws = _workspace(lib.sd_verify_tree_workspace_size(B, N, par, V), dev)
    a = _lib.sd_tree_args()
    a.batch, a.num_nodes, a.vocab = B, N, V
    a.parent = par
    a.target_rows = _ROW_PTRS(*t_ptrs)
    a.draft_rows = _ROW_PTRS(*d_ptrs)
    a.target_stride_b, a.draft_stride_b = t_stride, d_stride
    a.dtype = _DT[tdt]
    a.draft_tokens = draft_tokens.data_ptr()
    a.draft_tokens_stride_b = draft_tokens.stride(0) if B > 1 else draft_tokens.shape[1]
    a.proc = spec.struct()
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.pad_token = int(pad_token_id)
    a.noise = nz
    for f in TREE_FIELDS:
        setattr(a, f, getattr(out, f).data_ptr())
    a.path, a.path_stride_b = out.path.data_ptr(), depth
    if want_tokens:
        a.tokens_out, a.tokens_out_stride_b = out.tokens_out.data_ptr(), depth + 1
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_verify_tree(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify_tree")
    del keep
    return out


def verify_tree_distinct(target, draft_tokens: torch.Tensor, parent, proc, noise,
                         stop_tokens: Optional[torch.Tensor] = None, status_or: Optional[torch.Tensor] = None,
                         pad_token_id: int = 0, row_base: int = 0):
    """One token-tree verify step for DISTINCT children (sd_verify_tree_distinct): the children of a
    slot are distinct candidates fixed by the prefix (the drafter's top-c tokens, ``topk_children``),
    not iid draws, so no drafter row is read: child j of a slot is accepted with probability
    p[x_j] / (Z - the weights of the siblings rejected before it), and the emitted tokens keep the
    target's distribution exactly.  Under greedy a child is accepted iff its token is
    the row's maximum: the output is the target's greedy decode.

    target: [B, N+1, V] logits (or N+1 tensors [B, V]): slot 0 the root's row, slot i+1 the row after
    node i.  draft_tokens: int64 [B, >=N].  parent, proc, noise, stop_tokens, status_or, pad_token_id and
    the returned namespace are ``verify_tree``'s (resample_mass: the share of the row's mass left at a
    residual exit; n_sibling_rejects: the children rejected)."""
    from types import SimpleNamespace
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: verify_tree_distinct fuses the "
                        "processing of the target rows and cannot run a user _process")
    spec = proc_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_tree_distinct needs PhiloxNoise (the rule defines no stream order for this step)")
    tree = _tree_of(parent)
    N, depth = tree.num_nodes, tree.depth
    t_ptrs, t_stride, B, V, tdt, dev = _slot_rows(target, "target", list(range(N + 1)), N + 1, None)
    if not 1 <= B <= _lib.SD_TREE_MAX_BATCH:
        raise ValueError(f"verify_tree_distinct: batch must be in 1..{_lib.SD_TREE_MAX_BATCH}, got {B}")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != B \
            or draft_tokens.shape[1] < N or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B, >={N}] on {dev}")
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 device tensor")
    # one allocation: next_token (int64) first, then the six 4-byte fields and the path
    buf = torch.empty(8 * B + 4 * (6 + depth) * B, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    f4 = buf[8 * B:].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(6)]
    out = SimpleNamespace(n_accepted=i32[0], last_node=i32[1], next_token=nxt, resample_mass=i32[2].view(torch.float32),
                          n_sibling_rejects=i32[3], stop_index=i32[4], row_status=i32[5],
                          path=f4[6 * B:].view(B, depth),
                          tokens_out=torch.empty(B, depth + 1, dtype=torch.long, device=dev))
    nz, keep = _noise_struct(noise, 0, dev, row_base)
    par = getattr(tree, "_c_parent", None)
    if par is None:
        par = tree._c_parent = (C.c_int32 * _lib.SD_TREE_MAX_NODES)(*tree.parent)
    ws = _workspace(lib.sd_verify_tree_distinct_workspace_size(B, N, par, V), dev)
    a = _lib.sd_tree_distinct_args()
    a.batch, a.num_nodes, a.vocab = B, N, V
    a.parent = par
    a.target_rows = _ROW_PTRS(*t_ptrs)
    a.target_stride_b = t_stride
    a.dtype = _DT[tdt]
    a.draft_tokens = draft_tokens.data_ptr()
    a.draft_tokens_stride_b = draft_tokens.stride(0) if B > 1 else draft_tokens.shape[1]
    a.proc = spec.struct()
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.pad_token = int(pad_token_id)
    a.noise = nz
    for f in TREE_FIELDS:
        setattr(a, f, getattr(out, f).data_ptr())
    a.path, a.path_stride_b = out.path.data_ptr(), depth
    a.tokens_out, a.tokens_out_stride_b = out.tokens_out.data_ptr(), depth + 1
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_verify_tree_distinct(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify_tree_distinct")
    del keep
    return out


def verify_tree_dynamic(target, draft_tokens: torch.Tensor, parent_dev: torch.Tensor, proc, noise, max_depth: int,
                        stop_tokens: Optional[torch.Tensor] = None, status_or: Optional[torch.Tensor] = None,
                        pad_token_id: int = 0, row_base: int = 0):
    """``verify_tree_distinct`` with one topology PER SEQUENCE, read from device memory
    (sd_verify_tree_dynamic): parent_dev int32 [B, >=N] holds every sequence's parents
    (``tree_select`` writes them), N = target.shape[1] - 1.  max_depth (1..32) sizes path [B, max_depth] and
    tokens_out [B, max_depth + 1].  The topology is validated on the device: a sequence whose parents
    are out of range, has more than 8 children under one slot or is deeper than max_depth gets
    SD_ROW_INVALID_DIST, n_accepted 0, next_token -1 and path -1.  Everything else is
    ``verify_tree_distinct``'s."""
    from types import SimpleNamespace
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: verify_tree_dynamic fuses the "
                        "processing of the target rows and cannot run a user _process")
    spec = proc_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_tree_dynamic needs PhiloxNoise (the rule defines no stream order for this step)")
    if torch.is_tensor(target):
        if target.dim() != 3 or target.shape[1] < 2:
            raise ValueError(f"target: expected [B, N+1, V], got {tuple(target.shape)}")
        N = target.shape[1] - 1
    else:
        target = list(target)
        N = len(target) - 1
    depth = int(max_depth)
    if not 1 <= N <= _lib.SD_TREE_MAX_NODES:
        raise ValueError(f"verify_tree_dynamic: 1..{_lib.SD_TREE_MAX_NODES} nodes, got {N}")
    if not 1 <= depth <= _lib.SD_MAX_GAMMA:
        raise ValueError(f"verify_tree_dynamic: max_depth must be in 1..{_lib.SD_MAX_GAMMA}, got {depth}")
    t_ptrs, t_stride, B, V, tdt, dev = _slot_rows(target, "target", list(range(N + 1)), N + 1, None)
    if not 1 <= B <= _lib.SD_TREE_MAX_BATCH:
        raise ValueError(f"verify_tree_dynamic: batch must be in 1..{_lib.SD_TREE_MAX_BATCH}, got {B}")
    if draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 or draft_tokens.shape[0] != B \
            or draft_tokens.shape[1] < N or draft_tokens.stride(1) != 1 or draft_tokens.device != dev:
        raise ValueError(f"draft_tokens must be int64 [B, >={N}] on {dev}")
    if parent_dev.dtype != torch.int32 or parent_dev.dim() != 2 or parent_dev.shape[0] != B \
            or parent_dev.shape[1] < N or parent_dev.stride(1) != 1 or parent_dev.device != dev:
        raise ValueError(f"parent_dev must be int32 [B, >={N}] on {dev}")
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 device tensor")
    # one allocation: next_token (int64) first, then the six 4-byte fields and the path
    buf = torch.empty(8 * B + 4 * (6 + depth) * B, dtype=torch.uint8, device=dev)
    nxt = buf[:8 * B].view(torch.long)
    f4 = buf[8 * B:].view(torch.int32)
    i32 = [f4[k * B:(k + 1) * B] for k in range(6)]
    out = SimpleNamespace(n_accepted=i32[0], last_node=i32[1], next_token=nxt, resample_mass=i32[2].view(torch.float32),
                          n_sibling_rejects=i32[3], stop_index=i32[4], row_status=i32[5],
                          path=f4[6 * B:].view(B, depth),
                          tokens_out=torch.empty(B, depth + 1, dtype=torch.long, device=dev))
    nz, keep = _noise_struct(noise, 0, dev, row_base)
    ws = _workspace(lib.sd_verify_tree_dynamic_workspace_size(B, N, V), dev)
    a = _lib.sd_tree_dynamic_args()
    a.batch, a.num_nodes, a.vocab, a.max_depth = B, N, V, depth
    a.parent_dev = parent_dev.data_ptr()
    a.parent_stride_b = parent_dev.stride(0) if B > 1 else parent_dev.shape[1]
    a.target_rows = _ROW_PTRS(*t_ptrs)
    a.target_stride_b = t_stride
    a.dtype = _DT[tdt]
    a.draft_tokens = draft_tokens.data_ptr()
    a.draft_tokens_stride_b = draft_tokens.stride(0) if B > 1 else draft_tokens.shape[1]
    a.proc = spec.struct()
    a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
    a.pad_token = int(pad_token_id)
    a.noise = nz
    for f in TREE_FIELDS:
        setattr(a, f, getattr(out, f).data_ptr())
    a.path, a.path_stride_b = out.path.data_ptr(), depth
    a.tokens_out, a.tokens_out_stride_b = out.tokens_out.data_ptr(), depth + 1
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_verify_tree_dynamic(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_verify_tree_dynamic")
    del keep
    return out


# --------------------------------------------------------------------------- dynamic draft trees
def tree_pool(batch: int, pool_size: int, device):
    """The pool buffers ``tree_grow`` appends to and ``tree_select`` reads: a namespace of token int64,
    score fp32 and parent int32, each [batch, pool_size]."""
    from types import SimpleNamespace
    return SimpleNamespace(token=torch.zeros(batch, pool_size, dtype=torch.long, device=device),
                           score=torch.zeros(batch, pool_size, dtype=torch.float32, device=device),
                           parent=torch.zeros(batch, pool_size, dtype=torch.int32, device=device))


def _pool_check(pool, B: int, need: int, dev) -> int:
    for name, dt in (("token", torch.long), ("score", torch.float32), ("parent", torch.int32)):
        t = getattr(pool, name)
        if t.dtype != dt or t.dim() != 2 or t.shape[0] != B or t.shape[1] < need or t.stride(1) != 1 or t.device != dev:
            raise ValueError(f"pool.{name} must be {dt} [B, >={need}] on {dev}")
    st = pool.token.stride(0)
    if pool.score.stride(0) != st or pool.parent.stride(0) != st:
        raise ValueError("the pool's three buffers must share one row stride")
    return st if B > 1 else pool.token.shape[1]


def tree_grow(logits: torch.Tensor, level: int, width: int, branch: int, pool, frontier_in: Optional[torch.Tensor] = None,
              status_or: Optional[torch.Tensor] = None):
    """One level of a dynamic draft tree on the device (sd_tree_grow).  logits
    [B, F_prev, V]: the drafter's rows after the nodes of the current frontier (level 1: the root's one
    row), F_prev = ``DynamicTreeSpec.frontier[level - 1]``.  Every row's ``branch`` best tokens by raw
    logit become candidates with score = the parent's score + the fp32 log-softmax of the token; they
    are appended to ``pool`` (``tree_pool``) and the best min(width, F_prev * branch) of them form the next
    frontier, in ascending pool index.  frontier_in: the previous call's ``pool`` output int32 [B, F_prev]
    (None at level 1).  Returns a namespace of token int64, pool int32 and parent_rank int32, each
    [B, F_next], and row_status int32 [B].  No host synchronisation; a NaN row sets SD_ROW_INVALID_DIST."""
    from types import SimpleNamespace
    from .tree import DynamicTreeSpec
    if logits.dim() != 3:
        raise ValueError(f"logits: expected [B, F, V], got {tuple(logits.shape)}")
    B, F, V = logits.shape
    level, width, branch = int(level), int(width), int(branch)
    shape = DynamicTreeSpec(level, width, branch, 1)          # ValueError for a shape outside the limits
    if branch > V:
        raise ValueError(f"tree_grow: branch {branch} exceeds the vocabulary {V}")
    Fp, Fn, base = shape.frontier[level - 1], shape.frontier[level], shape.base[level - 1]
    if F != Fp:
        raise ValueError(f"logits: level {level} expands {Fp} frontier rows, got {F}")
    _require_rows(logits[:, 0, :], "logits", V)
    dev = logits.device
    if not 1 <= B <= _lib.SD_TREE_MAX_BATCH or V > _lib.SD_TREE_GROW_MAX_VOCAB:
        raise ValueError("tree_grow: batch or vocabulary outside the limits")
    pstride = _pool_check(pool, B, base + Fp * branch, dev)
    a = _lib.sd_tree_grow_args()
    if level > 1:
        if frontier_in is None or frontier_in.dtype != torch.int32 or frontier_in.dim() != 2 or frontier_in.shape[0] != B \
                or frontier_in.shape[1] < Fp or frontier_in.stride(1) != 1 or frontier_in.device != dev:
            raise ValueError(f"frontier_in must be int32 [B, >={Fp}] on {dev}")
        a.frontier_in = frontier_in.data_ptr()
        a.frontier_in_stride_b = frontier_in.stride(0) if B > 1 else frontier_in.shape[1]
    # one allocation: the tokens (int64) first, then pool, parent_rank and row_status
    buf = torch.empty(8 * B * Fn + 4 * (2 * B * Fn + B), dtype=torch.uint8, device=dev)
    f4 = buf[8 * B * Fn:].view(torch.int32)
    out = SimpleNamespace(token=buf[:8 * B * Fn].view(torch.long).view(B, Fn), pool=f4[:B * Fn].view(B, Fn),
                          parent_rank=f4[B * Fn:2 * B * Fn].view(B, Fn), row_status=f4[2 * B * Fn:])
    ws = _workspace(lib.sd_tree_grow_workspace_size(B, V, level, width, branch), dev)
    a.batch, a.vocab, a.level, a.width, a.branch, a.dtype = B, V, level, width, branch, _DT[logits.dtype]
    a.logits = logits.data_ptr()
    a.stride_b = logits.stride(0) if B > 1 else 0
    a.stride_r = logits.stride(1) if Fp > 1 else V
    a.pool_token, a.pool_score, a.pool_parent = pool.token.data_ptr(), pool.score.data_ptr(), pool.parent.data_ptr()
    a.pool_stride_b = pstride
    a.frontier_token, a.frontier_pool = out.token.data_ptr(), out.pool.data_ptr()
    a.frontier_parent_rank, a.frontier_stride_b = out.parent_rank.data_ptr(), Fn
    a.row_status = out.row_status.data_ptr()
    a.status_or = _status_or_ptr(status_or, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.sd_tree_grow(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_tree_grow")
    return out


def tree_select(pool, num_nodes: int, pool_size: Optional[int] = None, status_or: Optional[torch.Tensor] = None):
    """The rerank of a grown pool (sd_tree_select): the ``num_nodes`` best of the first ``pool_size`` entries
    (default: all) by (score descending, pool index ascending), in ascending pool index — a set closed
    under parents with parent[i] < i, what ``verify_tree_dynamic`` takes.  Returns a namespace of
    tokens int64, parent int32 (-1: a child of the root), depth int32 (1-based), pool_index int32 and
    anc int64 (bit k set iff node k is node i or an ancestor of it; the uint64 bit pattern), each [B, N],
    and row_status int32 [B]."""
    from types import SimpleNamespace
    B = pool.token.shape[0]
    P = pool.token.shape[1] if pool_size is None else int(pool_size)
    N = int(num_nodes)
    dev = pool.token.device
    if not 1 <= P <= _lib.SD_TREE_POOL_MAX:
        raise ValueError(f"tree_select: pool_size must be in 1..{_lib.SD_TREE_POOL_MAX}, got {P}")
    if not 1 <= N <= min(P, _lib.SD_TREE_MAX_NODES):
        raise ValueError(f"tree_select: num_nodes must be in 1..{min(P, _lib.SD_TREE_MAX_NODES)}, got {N}")
    if not 1 <= B <= _lib.SD_TREE_MAX_BATCH:
        raise ValueError("tree_select: batch outside the limits")
    pstride = _pool_check(pool, B, P, dev)
    # one allocation: tokens and anc (8-byte) first, then parent, depth, pool_index and row_status
    buf = torch.empty(16 * B * N + 4 * (3 * B * N + B), dtype=torch.uint8, device=dev)
    i8 = buf[:16 * B * N].view(torch.long)
    f4 = buf[16 * B * N:].view(torch.int32)
    out = SimpleNamespace(tokens=i8[:B * N].view(B, N), anc=i8[B * N:].view(B, N), parent=f4[:B * N].view(B, N),
                          depth=f4[B * N:2 * B * N].view(B, N), pool_index=f4[2 * B * N:3 * B * N].view(B, N),
                          row_status=f4[3 * B * N:])
    ws = _workspace(lib.sd_tree_select_workspace_size(B, P, N), dev)
    a = _lib.sd_tree_select_args()
    a.batch, a.pool_size, a.num_nodes = B, P, N
    a.pool_token, a.pool_score, a.pool_parent = pool.token.data_ptr(), pool.score.data_ptr(), pool.parent.data_ptr()
    a.pool_stride_b = pstride
    a.tokens, a.parent, a.depth = out.tokens.data_ptr(), out.parent.data_ptr(), out.depth.data_ptr()
    a.pool_index, a.anc, a.out_stride_b = out.pool_index.data_ptr(), out.anc.data_ptr(), N
    a.row_status = out.row_status.data_ptr()
    a.status_or = _status_or_ptr(status_or, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.sd_tree_select(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_tree_select")
    return out


def topk_children(logits_rows: torch.Tensor, k: int) -> torch.Tensor:
    """The k best token ids of every row of logits [R, V], int64 [R, k]: value descending, lowest index
    first among equals (one ``beam_topk`` pass).  These are the children ``verify_tree_distinct`` takes:
    the top-k of the raw logits is the top-k under any temperature and softmax, so no processor is
    applied.  R <= 64, k <= 64."""
    return beam_topk(logits_rows, int(k))[1]


# --------------------------------------------------------------------------- KV-cache compaction
def kv_compact(tensors, path: torch.Tensor, count: torch.Tensor, base: int, *, num_slots: int, node_slot=None,
               base_dev: Optional[torch.Tensor] = None, status_or: Optional[torch.Tensor] = None) -> None:
    """Move the accepted path of a token tree to the front of its cache window, in place
    (sd_kv_compact): in every tensor of ``tensors`` (the K and V buffers [B, H, L, D] of all layers: one
    shape, dtype and stride set, unit stride along D), for every sequence b and depth
    d < min(count[b], path.shape[1]) in ascending d, position ``base + slot(path[b, d])`` is copied to
    ``base + d``.  path: int32 [B, depth] and count: int32 [B] on the device, as ``verify_tree``
    returns them (``path``, ``n_accepted``): nothing is read back.  slot(i) is ``node_slot[i]`` (a host
    sequence: node index -> the order in which the node entered the cache) or i.  base_dev: an int64
    device tensor of one element added to ``base`` when the kernel runs (a StaticLayer's
    ``cumulative_length``), so a captured step needs no host value.  Only positions
    [base, base + num_slots) are read or written; a path entry that leaves the window ends its
    sequence's moves and ORs SD_ROW_INVALID_DIST into ``status_or``.  More than SD_KV_MAX_TENSORS
    tensors take one launch per 256, on the current stream."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("kv_compact: no tensors")
    t0 = tensors[0]
    if t0.dim() != 4:
        raise ValueError(f"kv_compact: expected [B, H, L, D] tensors, got {tuple(t0.shape)}")
    for t in tensors:
        if t.shape != t0.shape or t.dtype != t0.dtype or t.stride() != t0.stride() or t.device != t0.device:
            raise ValueError("kv_compact: the tensors must share one shape, dtype, stride set and device")
    if t0.stride(3) != 1:
        raise ValueError("kv_compact: the last dimension must have unit stride")
    B, H, L, D = t0.shape
    es, dev = t0.element_size(), t0.device
    if (D * es) % 2:
        raise ValueError("kv_compact: rows of an odd number of bytes are not supported")
    if not t0.is_cuda:
        raise ValueError("kv_compact: the tensors must be device tensors")
    if path.dtype != torch.int32 or path.dim() != 2 or path.shape[0] != B or path.stride(1) != 1 or path.device != dev \
            or not 1 <= path.shape[1] <= _lib.SD_MAX_GAMMA:
        raise ValueError(f"kv_compact: path must be int32 [B, 1..{_lib.SD_MAX_GAMMA}] on {dev}")
    if count.dtype != torch.int32 or count.shape != (B,) or count.device != dev or not count.is_contiguous():
        raise ValueError(f"kv_compact: count must be a contiguous int32 [B] on {dev}")
    num_slots, base = int(num_slots), int(base)
    if not 1 <= num_slots <= min(_lib.SD_TREE_MAX_NODES, L):
        raise ValueError(f"kv_compact: num_slots must be in 1..{min(_lib.SD_TREE_MAX_NODES, L)}, got {num_slots}")
    if base_dev is None:
        if not 0 <= base <= L - num_slots:
            raise ValueError(f"kv_compact: positions [{base}, {base + num_slots}) leave the cache's {L}")
    elif base_dev.dtype != torch.int64 or base_dev.numel() != 1 or base_dev.device != dev:
        raise ValueError("kv_compact: base_dev must be an int64 tensor of one element on the tensors' device")
    slots = None
    if node_slot is not None:
        node_slot = [int(s) for s in node_slot]
        if len(node_slot) > _lib.SD_TREE_MAX_NODES:
            raise ValueError(f"kv_compact: node_slot has at most {_lib.SD_TREE_MAX_NODES} entries")
        slots = (C.c_int32 * _lib.SD_TREE_MAX_NODES)(*(node_slot + [-1] * (_lib.SD_TREE_MAX_NODES - len(node_slot))))
    a = _lib.sd_kv_compact_args()
    a.batch, a.heads, a.max_depth, a.num_slots, a.row_bytes = B, H, path.shape[1], num_slots, D * es
    a.stride_b, a.stride_h, a.stride_pos = (t0.stride(0) * es if B > 1 else 0), t0.stride(1) * es, t0.stride(2) * es
    a.num_positions, a.base = L, base
    a.base_dev = base_dev.data_ptr() if base_dev is not None else None
    a.path, a.path_stride_b = path.data_ptr(), (path.stride(0) if B > 1 else path.shape[1])
    a.count = count.data_ptr()
    if slots is not None:
        a.node_slot = slots
    a.status_or = _status_or_ptr(status_or, dev)
    stream = C.c_void_p(_stream_ptr(dev))
    for i in range(0, len(tensors), _lib.SD_KV_MAX_TENSORS):
        part = tensors[i:i + _lib.SD_KV_MAX_TENSORS]
        table = (C.c_void_p * len(part))(*(t.data_ptr() for t in part))
        a.n_tensors, a.tensors = len(part), table
        _lib.check(lib.sd_kv_compact(C.byref(a), stream), "sd_kv_compact")


# --------------------------------------------------------------------------- n-gram verify (A11)
@dataclass
class NgramOut:
    n_accepted: torch.Tensor      # int32 [B]
    next_token: torch.Tensor      # int64 [B] (-1: a stop token among the accepted drafts)
    prune_target: torch.Tensor    # int32 [B]
    stop_index: torch.Tensor      # int32 [B]
    row_status: torch.Tensor      # int32 [B]
    filler_ids: Optional[torch.Tensor]   # int64 [B, γ'+1, K]
    words_used: torch.Tensor      # int64 [1]


def ngram_verify(target_rows: Sequence[torch.Tensor], draft_tokens: Optional[torch.Tensor], proc, noise,
                 stop_tokens: Optional[torch.Tensor] = None, filler_k: int = 0, sync_noise: bool = True,
                 row_base: int = 0, status_or: Optional[torch.Tensor] = None) -> NgramOut:
    """ngram_assisted/ngram_assisted.py:111-164 verify step for B sequences.

    target_rows: γ'+1 tensors [B, V] — rows 0..γ'-1 verify drafts 0..γ'-1, row γ' is the bonus row;
    draft_tokens: int64 [B, >=γ'] (None when γ' == 0).  Under StreamNoise the torch generator
    advances by the words the draws consumed (the reference's order), one device->host read."""
    spec = proc_spec(proc)
    target_rows = processed_rows(proc, list(target_rows))   # a user _process override (processed_rows)
    proc = spec
    gamma = len(target_rows) - 1
    if not 0 <= filler_k <= target_rows[0].shape[-1]:   # p.topk(k) raises for k > V as well
        raise ValueError(f"filler_k must be in [0, vocab = {target_rows[0].shape[-1]}]")
    if gamma > _lib.SD_MAX_GAMMA:   # the reference takes any γ: windows of <= SD_MAX_GAMMA drafts (chunked.py)
        from .chunked import ngram_verify_chunked
        return ngram_verify_chunked(target_rows, draft_tokens, proc, noise, stop_tokens, filler_k, sync_noise,
                                    row_base, status_or)
    if not 0 <= gamma:
        raise ValueError(f"gamma must be >= 0, got {gamma}")
    B, V = target_rows[0].shape
    dev = target_rows[0].device
    tdt = target_rows[0].dtype
    t_stride = target_rows[0].stride(0) if B > 1 else 0
    for i, t in enumerate(target_rows):
        _require_rows(t, f"target_rows[{i}]", V)
        if t.shape[0] != B or t.dtype != tdt or (B > 1 and t.stride(0) != t_stride):
            raise ValueError("target rows must share batch, dtype and batch stride")
    if gamma > 0:
        if draft_tokens is None or draft_tokens.dtype != torch.long or draft_tokens.shape[0] != B \
                or draft_tokens.shape[1] < gamma or draft_tokens.stride(1) != 1:
            raise ValueError("draft_tokens must be int64 [B, >=gamma] with a contiguous last axis")
        draft_tokens = draft_tokens.to(dev)
    if stop_tokens is None:
        stop_tokens = torch.empty(0, dtype=torch.long, device=dev)
    stop_tokens = stop_tokens.to(device=dev, dtype=torch.long).contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    out = NgramOut(torch.empty(B, **i32), torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, **i32),
                   torch.empty(B, **i32), torch.empty(B, **i32),
                   torch.empty(B, gamma + 1, filler_k, dtype=torch.long, device=dev) if filler_k else None,
                   torch.empty(1, dtype=torch.long, device=dev))
    need = B * (gamma + 1) * 2 * V if spec.stochastic else 0
    nz, keep = _noise_struct(noise, need, dev, row_base)
    ws = _workspace(lib.sd_ngram_workspace_size(B, gamma, V), dev)
    a = _lib.sd_ngram_args()
    a.batch, a.gamma, a.vocab = B, gamma, V
    for i, t in enumerate(target_rows):
        a.target_rows[i] = t.data_ptr()
    a.target_stride_b, a.target_dtype = t_stride, _DT[tdt]
    a.draft_tokens = draft_tokens.data_ptr() if gamma > 0 else None
    a.draft_tokens_stride_b = draft_tokens.stride(0) if gamma > 0 else 0
    a.proc, a.stop_tokens, a.n_stop, a.filler_k = spec.struct(), stop_tokens.data_ptr(), stop_tokens.numel(), filler_k
    a.noise = nz
    a.n_accepted, a.next_token = out.n_accepted.data_ptr(), out.next_token.data_ptr()
    a.prune_target, a.stop_index = out.prune_target.data_ptr(), out.stop_index.data_ptr()
    a.row_status, a.words_used = out.row_status.data_ptr(), out.words_used.data_ptr()
    a.filler_ids = out.filler_ids.data_ptr() if filler_k else None
    a.filler_stride_b = (gamma + 1) * filler_k
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.status_or = _status_or_ptr(status_or, dev)
    _lib.check(lib.sd_ngram_verify(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_ngram_verify")
    if isinstance(noise, StreamNoise) and sync_noise:
        noise.consumed(used_dev=out.words_used)
    del keep
    return out


# --------------------------------------------------------------------------- beam step (ABI 12)
def beam_length_penalty(length, alpha: float, min_length: float) -> float:
    """The reference's per-step divisor (sampling/base_decoding.py:106-107,165): the penalty in double,
    1 where it is 0, as the C float the kernel divides by."""
    lp = ((min_length + length) / (min_length + 1)) ** alpha
    return C.c_float(lp if lp != 0 else 1).value


def _beam_check_k(k: int, V: int) -> None:
    if not 1 <= k <= V:   # torch.topk's error, as the reference raises it (:128, :137)
        raise RuntimeError("selected index k out of range")


def beam_topk(logits: torch.Tensor, k: int, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """topk(log_softmax(logits, -1), k) of every row of logits [R, V] in one pass over the rows
    (k_beam_topk): (logprob fp32 [R, k] holding the value rounded to the logits dtype, token int64
    [R, k]), value descending, lowest index first among equal values.  R <= 64, k <= 64."""
    if logits.dim() != 2:
        raise ValueError(f"logits: expected [rows, vocab], got {tuple(logits.shape)}")
    R, V = logits.shape
    _require_rows(logits, "logits", V)
    _beam_check_k(int(k), V)
    dev = logits.device
    lp, tok = out if out is not None else (torch.empty(R, k, dtype=torch.float32, device=dev),
                                           torch.empty(R, k, dtype=torch.long, device=dev))
    ws = _workspace(lib.sd_beam_workspace_size(R, V, k), dev)
    a = _lib.sd_beam_args()
    a.mode, a.num_beams, a.top_k, a.vocab = _lib.SD_BEAM_TOPK_ONLY, R, int(k), V
    a.logits, a.stride_r, a.dtype = logits.data_ptr(), logits.stride(0), _DT[logits.dtype]
    a.top_logprob, a.top_token = lp.data_ptr(), tok.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.sd_beam_step(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_beam_step")
    return lp, tok


class BeamState:
    """The beam loop's state (sampling/base_decoding.py:115-119) as two device copies: a step reads
    one and writes the other (rows are permuted), then they swap.  ``input_ids`` / ``probs`` /
    ``beams_probs`` / ``last_indexes`` are the current copy; ``all_finished`` (int32 [1]) and ``parent``
    (int32 [num_beams, 2]: source beam, candidate index or -1) are what the last step wrote."""

    def __init__(self, input_ids: torch.Tensor, probs: torch.Tensor, beams_probs: torch.Tensor,
                 last_indexes: torch.Tensor):
        n, L = input_ids.shape
        dev = input_ids.device
        if not input_ids.is_cuda or input_ids.dtype != torch.long or probs.dtype != torch.float32 \
                or tuple(probs.shape) != (n, L) or beams_probs.dtype != torch.float32 or beams_probs.numel() != n \
                or last_indexes.dtype != torch.long or last_indexes.numel() != n \
                or any(t.device != dev for t in (probs, beams_probs, last_indexes)):
            raise ValueError("BeamState: input_ids int64 [n, L], probs fp32 [n, L], beams_probs fp32 [n], "
                             "last_indexes int64 [n], all on one GPU")
        cur = (input_ids.contiguous(), probs.contiguous(), beams_probs.contiguous(), last_indexes.contiguous())
        self._bufs = [cur, tuple(torch.empty_like(t) for t in cur)]
        self._cur = 0
        self.num_beams, self.total_len, self.device = n, L, dev
        self.all_finished = torch.zeros(1, dtype=torch.int32, device=dev)
        self.parent = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
        self.top_logprob = self.top_token = None

    @classmethod
    def start(cls, inputs: Sequence[int], num_beams: int, total_len: int, pad_token_id: int, device) -> "BeamState":
        """The reference's initial state (:115-125) for a prompt."""
        P = len(inputs)
        ids = torch.full((num_beams, total_len), pad_token_id, dtype=torch.long, device=device)
        ids[:, :P] = torch.tensor(inputs, dtype=torch.long, device=device)
        fmin = torch.finfo(torch.float).min
        probs = torch.full((num_beams, total_len), fmin, dtype=torch.float, device=device)
        probs[:, :P] = 1.0
        return cls(ids, probs, torch.full((num_beams,), 1.0, dtype=torch.float, device=device),
                   torch.full((num_beams,), -1, dtype=torch.long, device=device))

    input_ids = property(lambda self: self._bufs[self._cur][0])
    probs = property(lambda self: self._bufs[self._cur][1])
    beams_probs = property(lambda self: self._bufs[self._cur][2])
    last_indexes = property(lambda self: self._bufs[self._cur][3])


def beam_step(state: BeamState, logits: Optional[torch.Tensor], curr: int, *, top_k: int = 1, prefill: bool = False,
              length=None, alpha: float = 1.2, min_length: float = 5.0,
              stop_tokens: Optional[torch.Tensor] = None, pad_token_id: int = 0,
              topk: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """One step of beam_search_generate on the device (sd_beam_step): log_softmax + topk of the logit
    rows, the candidate loop, dedupe, stable sort and state update of sampling/base_decoding.py:
    136-178 (prefill=True: :127-131 on one row), written into ``state``'s other copy, which becomes
    current.  Returns the device word ``state.all_finished`` (1: every beam has finished; -1: fewer
    candidates than beams survived the dedupe, where the reference raises IndexError); nothing is read
    back here.  length: the penalty's length (default: 1 in the prefill).  topk=(logprob fp32 [R, K],
    token int64 [R, K]): select from these instead of reading ``logits`` (SD_BEAM_TOPK_GIVEN)."""
    n, L, dev = state.num_beams, state.total_len, state.device
    rows, K = (1, n) if prefill else (n, int(top_k))
    a = _lib.sd_beam_args()
    a.mode = _lib.SD_BEAM_PREFILL if prefill else _lib.SD_BEAM_STEP
    a.num_beams, a.top_k, a.curr, a.total_len = n, int(top_k), int(curr), L
    if not 1 <= curr < L:
        raise IndexError(f"index {curr} is out of bounds for dimension 1 with size {L}")
    if length is None:
        length = 1
    a.lp = beam_length_penalty(length, alpha, min_length)
    keep = None
    if topk is not None:
        lpv, tok = topk
        if lpv.dtype != torch.float32 or tok.dtype != torch.long or tuple(lpv.shape) != (rows, K) \
                or tuple(tok.shape) != (rows, K) or not lpv.is_contiguous() or not tok.is_contiguous() \
                or lpv.device != dev or tok.device != dev:
            raise ValueError(f"topk must be (fp32 [{rows}, {K}], int64 [{rows}, {K}]) contiguous on {dev}")
        a.flags = _lib.SD_BEAM_TOPK_GIVEN
        a.vocab = max(K, 1)
        state.top_logprob, state.top_token = lpv, tok
    else:
        if logits is None:
            raise ValueError("beam_step needs logits, or topk=(logprob, token) to select from")
        if logits.dim() != 2 or logits.shape[0] != rows:
            raise ValueError(f"logits: expected [{rows}, vocab], got {tuple(logits.shape)}")
        V = logits.shape[1]
        _require_rows(logits, "logits", V)
        _beam_check_k(K, V)
        if logits.device != dev:
            raise ValueError("logits and the beam state must share a device")
        a.vocab = V
        a.logits, a.stride_r, a.dtype = logits.data_ptr(), logits.stride(0), _DT[logits.dtype]
        if state.top_logprob is None or tuple(state.top_logprob.shape) != (rows, K):
            state.top_logprob = torch.empty(rows, K, dtype=torch.float32, device=dev)
            state.top_token = torch.empty(rows, K, dtype=torch.long, device=dev)
        nbytes = lib.sd_beam_workspace_size(rows, V, K)
        if nbytes:   # 0: a shape the library refuses; sd_beam_step reports which limit
            keep = _workspace(nbytes, dev)
            a.workspace, a.workspace_bytes = keep.data_ptr(), keep.numel()
    a.top_logprob, a.top_token = state.top_logprob.data_ptr(), state.top_token.data_ptr()
    stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
    if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
        raise ValueError("stop_tokens must be a contiguous int64 tensor on the state's device")
    a.stop_tokens, a.n_stop, a.pad_token = (stops.data_ptr() if stops.numel() else None), stops.numel(), int(pad_token_id)
    src, dst = state._bufs[state._cur], state._bufs[1 - state._cur]
    a.input_ids_in, a.input_ids_out, a.input_ids_stride = src[0].data_ptr(), dst[0].data_ptr(), L
    a.probs_in, a.probs_out, a.probs_stride = src[1].data_ptr(), dst[1].data_ptr(), L
    a.beams_probs_in, a.beams_probs_out = src[2].data_ptr(), dst[2].data_ptr()
    a.last_index_in, a.last_index_out = src[3].data_ptr(), dst[3].data_ptr()
    a.all_finished, a.parent = state.all_finished.data_ptr(), state.parent.data_ptr()
    _lib.check(lib.sd_beam_step(C.byref(a), C.c_void_p(_stream_ptr(dev))), "sd_beam_step")
    state._cur = 1 - state._cur
    del keep
    return state.all_finished
