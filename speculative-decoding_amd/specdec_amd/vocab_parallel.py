"""Vocabulary-parallel verify (sd_vp_stats / sd_vp_decide / sd_vp_finish, include/specdec.h; DESIGN.md
§4d): one SD_RULE_SPEC step on the logits as a tensor-parallel forward leaves them — every rank holds
a column slice of each row — with two all-gathers of a few hundred bytes per sequence in place of
the all-gather of the rows.

    shard = VocabShard.even(rank, world, vocab)
    out = verify_vocab_parallel(target_slices, draft_slices, draft_tokens, proc, noise, shard,
                                GroupExchange(group))

Every rank passes the same drafts, the same processor and a PhiloxNoise with the same seed and
offset; every rank then returns the same outputs, bit for bit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import lib
from .noise import PhiloxNoise
from .ops import _DT, _noise_struct, _status_or_ptr, _stream_ptr, _user_process, _workspace, proc_spec


@dataclass(frozen=True)
class VocabShard:
    """Shard `shard` of `num_shards` holds columns [vocab_offset, vocab_offset + vocab_local) of `vocab`."""
    shard: int
    num_shards: int
    vocab_offset: int
    vocab_local: int
    vocab: int

    def __post_init__(self):
        if not (0 <= self.shard < self.num_shards <= _lib.SD_VP_MAX_SHARDS):
            raise ValueError(f"VocabShard: shard {self.shard} of {self.num_shards} (at most {_lib.SD_VP_MAX_SHARDS})")
        if self.vocab_local < 1 or self.vocab_offset < 0 or self.vocab_offset + self.vocab_local > self.vocab:
            raise ValueError(f"VocabShard: [{self.vocab_offset}, {self.vocab_offset + self.vocab_local}) is no "
                             f"slice of [0, {self.vocab})")

    @classmethod
    def even(cls, rank: int, world: int, vocab: int) -> "VocabShard":
        """The contiguous split of a column-parallel linear: the first vocab % world shards hold one
        more column."""
        q, r = divmod(int(vocab), int(world))
        return cls(rank, world, rank * q + min(rank, r), q + (1 if rank < r else 0), vocab)

    @classmethod
    def split(cls, sizes: Sequence[int]) -> List["VocabShard"]:
        """All shards of a partition given its slice sizes (uneven splits)."""
        off, out = 0, []
        for s, n in enumerate(sizes):
            out.append(cls(s, len(sizes), off, int(n), int(sum(sizes))))
            off += int(n)
        return out

    def view(self, rows: torch.Tensor) -> torch.Tensor:
        """This shard's columns of whole rows [..., vocab]: a view, no copy."""
        return rows[..., self.vocab_offset:self.vocab_offset + self.vocab_local]


@dataclass
class VocabVerifyOut:
    n_accepted: torch.Tensor      # int32 [B]
    next_token: torch.Tensor      # int64 [B]
    resample_mass: torch.Tensor   # fp32  [B]
    prune_drafter: torch.Tensor   # int32 [B]
    prune_target: torch.Tensor    # int32 [B]
    stop_index: torch.Tensor      # int32 [B]
    row_status: torch.Tensor      # int32 [B]
    words_used: torch.Tensor      # int64 [1], always 0 (PhiloxNoise)
    owner_shard: torch.Tensor     # int32 [B]: the shard whose candidate was taken, -1 if none


VP_FIELDS = ("n_accepted", "next_token", "resample_mass", "prune_drafter", "prune_target", "stop_index",
             "row_status", "owner_shard")


# --------------------------------------------------------------------------- exchanges
def _check_gathered(t, S: int, nbytes: int, dev, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (S, nbytes) or t.device != dev \
            or not t.is_contiguous():
        got = (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"verify_vocab_parallel: the exchange of the {what} blocks must return a contiguous uint8 "
                         f"tensor [{S}, {nbytes}] on {dev}, got {got}")
    return t


class GroupExchange:
    """All-gather of one block per rank over a torch.distributed group, in rank order.  On a gloo
    group the few hundred bytes are staged through the host (device -> CPU -> all_gather -> device:
    one sync per exchange); on an RCCL group ``all_gather_into_tensor`` runs on the device bytes."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        self.host = dist.get_backend(group) == "gloo"

    def __call__(self, local: torch.Tensor) -> torch.Tensor:
        n = local.numel()
        if self.host:
            mine = local.detach().reshape(-1).cpu()
            parts = [torch.empty(n, dtype=torch.uint8) for _ in range(self.world)]
            self.dist.all_gather(parts, mine, group=self.group)
            return torch.stack(parts).to(local.device)
        out = torch.empty(self.world, n, dtype=torch.uint8, device=local.device)
        self.dist.all_gather_into_tensor(out, local.reshape(-1), group=self.group)
        return out


class LocalShards:
    """An EMULATION of S ranks for tests and timing on one GPU: the S shards of a step run in one
    process, on one device and stream, in lock step — phase 1 of every shard, the concatenation of
    their blocks in shard order, phase 3 of every shard, the concatenation, phase 5 of every shard.
    Nothing is exchanged between devices.  ``verify_vocab_parallel(..., shard=None, exchange=ls)``
    takes per-shard inputs (or whole rows, which are sliced as views) and returns one output per
    shard; a serving rank uses ``GroupExchange``."""

    def __init__(self, shards: Sequence[VocabShard]):
        self.shards = list(shards)
        S = len(self.shards)
        at = 0
        for s, sh in enumerate(self.shards):
            if sh.shard != s or sh.num_shards != S or sh.vocab_offset != at or sh.vocab != self.shards[0].vocab:
                raise ValueError("LocalShards: the shards must be shard 0..S-1 of one partition, in order")
            at += sh.vocab_local
        if at != self.shards[0].vocab:
            raise ValueError("LocalShards: the slices do not add up to the vocabulary")

    @classmethod
    def even(cls, world: int, vocab: int) -> "LocalShards":
        return cls([VocabShard.even(r, world, vocab) for r in range(world)])

    @staticmethod
    def concat(blocks: Sequence[torch.Tensor]) -> torch.Tensor:
        return torch.stack([b.reshape(-1) for b in blocks])

    def slices(self, rows):
        """Per-shard inputs from whole rows ([..., vocab] tensor or a sequence of them: views), or the
        per-shard sequence given."""
        V, S = self.shards[0].vocab, len(self.shards)
        if rows is None:
            return [None] * S
        if torch.is_tensor(rows):
            if rows.shape[-1] != V:
                raise ValueError(f"LocalShards: whole rows must have {V} columns, got {tuple(rows.shape)}")
            return [sh.view(rows) for sh in self.shards]
        rows = list(rows)
        if not rows:
            return [None] * S

        def width(r):
            r = r if torch.is_tensor(r) else (r[0] if r is not None and len(r) else None)
            return None if r is None else r.shape[-1]

        if len(rows) == S and all(width(r) in (None, sh.vocab_local) for r, sh in zip(rows, self.shards)):
            return rows                               # one entry per shard
        if all(torch.is_tensor(r) and r.shape[-1] == V for r in rows):
            return [[sh.view(r) for r in rows] for sh in self.shards]
        raise ValueError(f"LocalShards: expected whole rows of {V} columns or one entry per shard ({S})")

    def run(self, steps):
        """Drive S step generators (one per shard) in lock step; returns their results."""
        steps = list(steps)
        blocks = [next(g) for g in steps]
        while True:
            gathered = self.concat(blocks)
            blocks, done = [], []
            for g in steps:
                try:
                    blocks.append(g.send(gathered))
                except StopIteration as e:
                    done.append(e.value)
            if done:
                if len(done) != len(steps):
                    raise RuntimeError("LocalShards: the shards fell out of step")
                return done


# --------------------------------------------------------------------------- one shard's step
def _rows_of(x) -> list:
    if x is None:
        return []
    if torch.is_tensor(x):
        if x.dim() == 3:
            return [x[:, t, :] for t in range(x.shape[1])]
        if x.dim() == 2:
            return [x]
        raise ValueError(f"expected [B, rows, V_s] or [B, V_s], got {tuple(x.shape)}")
    return list(x)


def _slice_rows(x, n_rows: int, name: str, Vs: int):
    """(per-row tensors [B, Vs], batch stride) of a [B, n_rows, Vs] tensor or n_rows tensors [B, Vs]; views."""
    rows = _rows_of(x)
    if n_rows == 0 and not rows:
        return [], 0
    if len(rows) != n_rows:
        raise ValueError(f"{name}: expected {n_rows} rows, got {len(rows)}")
    B = rows[0].shape[0]
    stride = rows[0].stride(0) if B > 1 else 0
    for i, t in enumerate(rows):
        if t.dim() != 2 or t.shape != (B, Vs):
            raise ValueError(f"{name}[{i}]: expected [{B}, {Vs}] (the shard's slice), got {tuple(t.shape)}")
        if t.stride(1) != 1:
            raise ValueError(f"{name}[{i}]: the vocabulary axis must have unit stride")
        if not t.is_cuda or t.dtype not in _DT:
            raise ValueError(f"{name}[{i}]: must be a device tensor of a supported dtype")
        if B > 1 and t.stride(0) != stride:
            raise ValueError(f"{name}: the rows must share one batch stride")
    return rows, stride


_ZERO = {}


def _zero_word(dev) -> torch.Tensor:
    """An int64 [1] zero on dev (VocabVerifyOut.words_used: Philox noise consumes no words); shared,
    never written.  Inside a graph capture a fresh one is made (the cached one must not come from
    a graph's memory pool)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(1, dtype=torch.long, device=dev)
    z = _ZERO.get(dev)
    if z is None:
        z = _ZERO[dev] = torch.zeros(1, dtype=torch.long, device=dev)
    return z


class _Step:
    """One shard's step: the sd_vp_args of its three calls and the buffers they write."""

    def __init__(self, B: int, gamma: int, dev, dt, shard: VocabShard, spec, nz, trows=(), t_stride=0, drows=(),
                 d_stride=0, draft_tokens=None, stop_tokens=None, skip: bool = False, status_or=None):
        if not 1 <= B <= _lib.SD_VP_MAX_BATCH:
            raise ValueError(f"verify_vocab_parallel: batch {B} outside 1..{_lib.SD_VP_MAX_BATCH}")
        if not 0 <= gamma <= _lib.SD_MAX_GAMMA:
            raise ValueError(f"verify_vocab_parallel: gamma {gamma} outside 0..{_lib.SD_MAX_GAMMA}")
        if shard.vocab_local > _lib.SD_VP_MAX_VOCAB_LOCAL:
            raise ValueError(f"verify_vocab_parallel: a slice holds at most {_lib.SD_VP_MAX_VOCAB_LOCAL} columns")
        stops = stop_tokens if stop_tokens is not None else torch.empty(0, dtype=torch.long, device=dev)
        if stops.dtype != torch.long or stops.device != dev or not stops.is_contiguous():
            raise ValueError("stop_tokens must be a contiguous int64 device tensor")
        self.B, self.gamma, self.dev, self.S = B, gamma, dev, shard.num_shards
        self.nstat, self.ncand = lib.sd_vp_stats_bytes(B, gamma), lib.sd_vp_cand_bytes(B)
        ws = _workspace(lib.sd_vp_workspace_size(B, gamma, shard.vocab_local), dev)
        a = _lib.sd_vp_args()
        a.batch, a.gamma, a.vocab, a.vocab_offset = B, gamma, shard.vocab, shard.vocab_offset
        a.vocab_local, a.shard, a.num_shards, a.dtype = shard.vocab_local, shard.shard, shard.num_shards, _DT[dt]
        for i, t in enumerate(trows):
            a.target_rows[i] = t.data_ptr()
        for i, t in enumerate(drows):
            a.draft_rows[i] = t.data_ptr()
        a.target_stride_b, a.draft_stride_b = t_stride, d_stride
        if gamma and draft_tokens is not None:
            a.draft_tokens, a.draft_tokens_stride_b = draft_tokens.data_ptr(), draft_tokens.stride(0)
        a.proc = spec.struct()
        a.skip_sample_adjustment = 1 if skip else 0
        a.stop_tokens, a.n_stop = (stops.data_ptr() if stops.numel() else None), stops.numel()
        a.noise = nz
        a.status_or = _status_or_ptr(status_or, dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        self.a = a
        self.keep = (trows, drows, draft_tokens, stops, ws, status_or)

    def _stream(self):
        return C.c_void_p(_stream_ptr(self.dev))

    def stats(self) -> torch.Tensor:
        out = torch.empty(self.nstat, dtype=torch.uint8, device=self.dev)
        self.a.stats_local = out.data_ptr()
        _lib.check(lib.sd_vp_stats(C.byref(self.a), self._stream()), "sd_vp_stats")
        return out

    def decide(self, stats_all) -> torch.Tensor:
        stats_all = _check_gathered(stats_all, self.S, self.nstat, self.dev, "statistics")
        out = torch.empty(self.ncand, dtype=torch.uint8, device=self.dev)
        self.a.stats_all, self.a.cand_local = stats_all.data_ptr(), out.data_ptr()
        _lib.check(lib.sd_vp_decide(C.byref(self.a), self._stream()), "sd_vp_decide")
        return out

    def finish(self, cand_all) -> VocabVerifyOut:
        cand_all = _check_gathered(cand_all, self.S, self.ncand, self.dev, "candidate")
        B = self.B
        # one allocation, every byte written by the kernel: next_token (int64) first, then the seven
        # 4-byte fields; words_used is a constant zero (no launch of its own)
        buf = torch.empty(8 * B + 4 * 7 * B, dtype=torch.uint8, device=self.dev)
        nxt, used = buf[:8 * B].view(torch.long), _zero_word(self.dev)
        f4 = buf[8 * B:].view(torch.int32)
        i32 = [f4[k * B:(k + 1) * B] for k in range(7)]
        out = VocabVerifyOut(i32[0], nxt, i32[1].view(torch.float32), i32[2], i32[3], i32[4], i32[5], used, i32[6])
        self.a.cand_all = cand_all.data_ptr()
        for f in VP_FIELDS:
            setattr(self.a, f, getattr(out, f).data_ptr())
        _lib.check(lib.sd_vp_finish(C.byref(self.a), self._stream()), "sd_vp_finish")
        return out


def _step_of(target_slices, draft_slices, draft_tokens, spec, nz, shard: VocabShard, stop_tokens=None,
             skip: bool = False, status_or=None) -> _Step:
    """Validate one shard's inputs (host only, before any launch) and build its step."""
    Vs = shard.vocab_local
    target_slices = _rows_of(target_slices)
    gamma = len(target_slices) - 1
    if not 0 <= gamma <= _lib.SD_MAX_GAMMA:
        raise ValueError(f"verify_vocab_parallel: gamma {gamma} outside 0..{_lib.SD_MAX_GAMMA}")
    trows, t_stride = _slice_rows(target_slices, gamma + 1, "target_slices", Vs)
    drows, d_stride = _slice_rows(draft_slices, gamma, "draft_slices", Vs)
    B, dev, dt = trows[0].shape[0], trows[0].device, trows[0].dtype
    for t in trows + drows:
        if t.shape[0] != B or t.dtype != dt or t.device != dev:
            raise ValueError("target and draft slices must share batch, dtype and device")
    if gamma:
        if draft_tokens is None or draft_tokens.dtype != torch.long or draft_tokens.dim() != 2 \
                or draft_tokens.shape[0] != B or draft_tokens.shape[1] < gamma or draft_tokens.stride(1) != 1 \
                or draft_tokens.device != dev:
            raise ValueError(f"draft_tokens must be int64 [B, >={gamma}] on {dev}")
    return _Step(B, gamma, dev, dt, shard, spec, nz, trows, t_stride, drows, d_stride, draft_tokens, stop_tokens, skip,
                 status_or)


def _vp_step(target_slices, draft_slices, draft_tokens, spec, nz, shard: VocabShard, stop_tokens, skip: bool,
             status_or):
    """Generator: yields the shard's statistics block, takes the gathered blocks, yields the candidate
    block, takes the gathered blocks, returns VocabVerifyOut."""
    st = _step_of(target_slices, draft_slices, draft_tokens, spec, nz, shard, stop_tokens, skip, status_or)
    stats_all = yield st.stats()
    cand_all = yield st.decide(stats_all)
    return st.finish(cand_all)


def _vp_spec(proc):
    if _user_process(proc) is not None:
        raise TypeError(f"unsupported logits processor {type(proc).__name__}: the vocabulary-parallel verify processes "
                        "slices of the rows and cannot run a user _process")
    spec = proc_spec(proc)
    if spec.keeps:
        raise TypeError(f"unsupported logits processor {spec.kind}: the vocabulary-parallel verify takes greedy and "
                        "multinomial processors only (no top-k / nucleus search over slices)")
    return spec


def verify_vocab_parallel(target_slices, draft_slices, draft_tokens: Optional[torch.Tensor], proc, noise,
                          shard: Optional[VocabShard], exchange, stop_tokens: Optional[torch.Tensor] = None,
                          row_base: int = 0, skip_sample_adjustment: bool = False,
                          status_or: Optional[torch.Tensor] = None):
    """One vocabulary-parallel SD_RULE_SPEC verify step of B sequences on this rank's slices.

    target_slices: [B, γ+1, V_s] logits (or γ+1 tensors [B, V_s]) — columns shard.vocab_offset.. of
    the target rows; draft_slices: [B, γ, V_s] (or γ tensors; None when γ = 0: "sample the one target
    row").  Views into wider rows are taken as they are (only the vocabulary axis needs unit stride):
    a replicated drafter's full rows are passed as ``row[..., off:off + V_s]``.  draft_tokens: int64
    [B, >=γ], GLOBAL ids, the same on every rank.  proc: greedy or multinomial, any temperature.
    noise: PhiloxNoise, the same seed and offset on every rank (one offset per step).
    exchange(local uint8 [nbytes]) -> uint8 [S, nbytes]: the all-gather of one block per rank, in rank
    order (``GroupExchange``); called twice per step.
    Returns VocabVerifyOut: ``ops.VerifyOut``'s fields plus owner_shard; every rank gets the same bits.

    With ``exchange`` a ``LocalShards`` (single-GPU emulation; shard=None) the slices are one entry
    per shard, or whole rows [..., V] that are sliced as views, and the result is one VocabVerifyOut
    per shard."""
    spec = _vp_spec(proc)
    if not isinstance(noise, PhiloxNoise):
        raise TypeError("verify_vocab_parallel needs PhiloxNoise (SD_NOISE_STREAM's draw order needs whole rows)")
    if isinstance(exchange, LocalShards):
        ts, ds = exchange.slices(target_slices), exchange.slices(draft_slices)
        first = ts[0] if torch.is_tensor(ts[0]) else ts[0][0]
        nz, keep = _noise_struct(noise, 0, first.device, row_base)
        outs = exchange.run(_vp_step(ts[s], ds[s], draft_tokens, spec, nz, sh, stop_tokens, skip_sample_adjustment,
                                     status_or) for s, sh in enumerate(exchange.shards))
        del keep
        return outs
    if not isinstance(shard, VocabShard):
        raise TypeError("verify_vocab_parallel: shard must be a VocabShard")
    first = target_slices if torch.is_tensor(target_slices) else target_slices[0]
    nz, keep = _noise_struct(noise, 0, first.device, row_base)
    step = _vp_step(target_slices, draft_slices, draft_tokens, spec, nz, shard, stop_tokens, skip_sample_adjustment,
                    status_or)
    block = next(step)
    while True:
        try:
            block = step.send(exchange(block))
        except StopIteration as e:
            del keep
            return e.value
