"""torch.library registration of the hot-path entry points ("wrapped by
torch.library ops"), so the sampler and the verify step are dispatcher-visible operators —
traceable by torch.compile / torch.export (fake implementations give output shapes without a
GPU), and callable as ``torch.ops.specdec.*``.

    torch.ops.specdec.sample(logits [R, V], kind, temperature, top_k, top_p, seed, offset, row_base)
        -> (tokens int64 [R], row_stats fp32 [R, 2], row_status int32 [R])
        LogitsProcessor.__call__ + .sample per row (utils/logits_processor.py:13-103), Philox noise.
    torch.ops.specdec.verify(target [B, T, V], draft [B, γ, V], draft_tokens int64 [B, >=γ], stop_tokens int64 [n],
                             rule, kind, temperature, top_k, top_p, seed, offset, row_base)
        -> (n_accepted int32 [B], next_token int64 [B], resample_mass fp32 [B], prune_drafter int32 [B],
            prune_target int32 [B], stop_index int32 [B], row_status int32 [B])
        One verify step: rule 0 = sampling/speculative_decoding.py:129-187 (T = γ+1 target rows),
        rule 1 = engine/infer_engine.py:276-336 (T = γ, plain softmax), Philox noise.

    torch.ops.specdec.verify_multi(target [B, K, γ+1, V], draft [B, K, γ, V], draft_tokens int64 [B, K, >=γ],
                                   stop_tokens int64 [n], kind, temperature, top_k, top_p, seed, offset, row_base)
        -> (n_accepted, winner int32 [B], next_token int64 [B], resample_mass fp32 [B], n_sibling_rejects,
            prune_drafter, prune_target, stop_index, row_status int32 [B])
        One multi-draft verify step over K chains per sequence (sd_verify_multi), Philox noise.

    torch.ops.specdec.verify_block(target [B, γ+1, V], draft [B, γ, V], draft_tokens int64 [B, >=γ],
                                   stop_tokens int64 [n], kind, temperature, top_k, top_p, seed, offset, row_base)
        -> (n_accepted int32 [B], next_token int64 [B], resample_mass fp32 [B], prune_drafter, prune_target,
            stop_index, row_status int32 [B], weights fp32 [B, γ+1], accept_prob fp32 [B, γ])
        One block verify step (sd_verify_block): the drafted block verified jointly, Philox noise.

    torch.ops.specdec.verify_tree(target [B, N+1, V], draft [B, I, V], draft_tokens int64 [B, >=N], parent int[N],
                                  stop_tokens int64 [n], kind, temperature, top_k, top_p, seed, offset, row_base)
        -> (n_accepted, last_node int32 [B], next_token int64 [B], resample_mass fp32 [B], n_sibling_rejects,
            stop_index, row_status int32 [B], path int32 [B, depth])
        One token-tree verify step (sd_verify_tree): N nodes with parents `parent`, the I internal slots'
        drafter rows in ascending slot order, Philox noise.

    torch.ops.specdec.verify_tree_distinct(target [B, N+1, V], draft_tokens int64 [B, >=N], parent int[N],
                                           stop_tokens int64 [n], kind, temperature, top_k, top_p, seed, offset,
                                           row_base) -> the same outputs as verify_tree
        One token-tree verify step whose children are distinct candidates, e.g. the drafter's top-c tokens
        (sd_verify_tree_distinct): no drafter rows, Philox noise.

    torch.ops.specdec.tree_grow(logits [B, F, V], level, width, branch, pool_token int64 [B, P], pool_score fp32 [B, P],
                                pool_parent int32 [B, P], frontier_in int32 [B, F]?)
        -> (frontier_token int64 [B, F'], frontier_pool int32 [B, F'], frontier_parent_rank int32 [B, F'],
            row_status int32 [B])
        One level of a dynamic draft tree (sd_tree_grow): appends the level's candidates to the pool (mutated).
    torch.ops.specdec.tree_select(pool_token, pool_score, pool_parent, num_nodes, pool_size)
        -> (tokens int64, parent int32, depth int32, pool_index int32, anc int64 [B, N], row_status int32 [B])
        The rerank (sd_tree_select): the N best pool entries in ascending pool index.
    torch.ops.specdec.verify_tree_dynamic(target [B, N+1, V], draft_tokens int64 [B, >=N], parent_dev int32 [B, >=N],
                                          max_depth, stop_tokens int64 [n], kind, temperature, top_k, top_p, seed,
                                          offset, row_base) -> verify_tree's outputs, path int32 [B, max_depth]
        verify_tree_distinct with one topology per sequence, read from device memory (sd_verify_tree_dynamic).

    torch.ops.specdec.beam_topk(logits [R, V], k) -> (logprob fp32 [R, k], token int64 [R, k])
        The beam step's row pass: topk(log_softmax(logits), k), lowest index first among equal values
        (sampling/base_decoding.py:136-137).

    torch.ops.specdec.vp_stats(target [B, γ+1, V_s], draft [B, γ, V_s], draft_tokens int64 [B, >=γ], shard,
                               num_shards, vocab_offset, vocab, kind, temperature) -> stats block uint8 [n]
    torch.ops.specdec.vp_decide(target, draft, draft_tokens, stop_tokens, stats_all uint8 [S, n], shard, num_shards,
                                vocab_offset, vocab, kind, temperature, skip_sample_adjustment, seed, offset,
                                row_base) -> candidate block uint8 [m]
    torch.ops.specdec.vp_finish(cand_all uint8 [S, m], gamma, shard, num_shards, vocab_offset, vocab_local, vocab,
                                kind, seed, offset, row_base)
        -> (n_accepted int32 [B], next_token int64 [B], resample_mass fp32 [B], prune_drafter, prune_target,
            stop_index, row_status, owner_shard int32 [B])
        The three phases of the vocabulary-parallel verify on one rank's slices (sd_vp_stats / sd_vp_decide /
        sd_vp_finish; specdec_amd.vocab_parallel); the caller all-gathers the blocks between them.

    torch.ops.specdec.kv_compact(tensors Tensor[] ([B, H, L, D] each), path int32 [B, depth], count int32 [B], base,
                                 num_slots, node_slot int[]?, base_dev int64 [1]?) -> ()
        KV-cache compaction onto the accepted path (sd_kv_compact), in place: in every tensor, position
        base + slot(path[b, d]) moves to base + d for d < count[b].  Mutates `tensors`; the sticky error
        word (status_or) stays on the Python API, ops.kv_compact.

All run the same C-ABI calls as ``specdec_amd.ops`` (libspecdec.so); the parity STREAM noise
mode keeps generator state on the host side and stays on the Python API.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ops
from . import vocab_parallel as vp
from .noise import PhiloxNoise

_KINDS = {v: k for k, v in ops.KIND.items()}


def _spec(kind: int, temperature: float, top_k: int, top_p: float) -> ops.ProcSpec:
    if kind not in _KINDS:
        raise ValueError(f"unknown processor kind {kind}")
    return ops.ProcSpec(_KINDS[kind], float(temperature), int(top_k), float(top_p))


@torch.library.custom_op("specdec::sample", mutates_args=())
def sample(logits: Tensor, kind: int, temperature: float, top_k: int, top_p: float, seed: int, offset: int,
           row_base: int) -> Tuple[Tensor, Tensor, Tensor]:
    R = logits.shape[0]
    stats = torch.empty(R, 2, dtype=torch.float32, device=logits.device)
    tokens, _, status = ops.sample_rows(logits, _spec(kind, temperature, top_k, top_p),
                                        PhiloxNoise(seed, offset), row_base=row_base, row_stats_out=stats)
    return tokens, stats, status


@sample.register_fake
def _(logits, kind, temperature, top_k, top_p, seed, offset, row_base):
    R = logits.shape[0]
    return (logits.new_empty(R, dtype=torch.long), logits.new_empty(R, 2, dtype=torch.float32),
            logits.new_empty(R, dtype=torch.int32))


@torch.library.custom_op("specdec::verify", mutates_args=())
def verify(target: Tensor, draft: Tensor, draft_tokens: Tensor, stop_tokens: Tensor, rule: int, kind: int,
           temperature: float, top_k: int, top_p: float, seed: int, offset: int,
           row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    gamma = draft.shape[1]
    spec = _spec(kind, temperature, top_k, top_p) if rule == _lib.SD_RULE_SPEC else ops.PLAIN_SOFTMAX
    out = ops.verify([target[:, t] for t in range(target.shape[1])], [draft[:, d] for d in range(gamma)],
                     draft_tokens, rule, spec, spec, PhiloxNoise(seed, offset), stop_tokens, row_base=row_base)
    # ops.verify hands back views of one device buffer; a custom op's outputs may not alias each other
    return tuple(t.clone() for t in (out.n_accepted, out.next_token, out.resample_mass, out.prune_drafter,
                                     out.prune_target, out.stop_index, out.row_status))


@verify.register_fake
def _(target, draft, draft_tokens, stop_tokens, rule, kind, temperature, top_k, top_p, seed, offset, row_base):
    B = target.shape[0]
    i32 = dict(dtype=torch.int32)
    return (target.new_empty(B, **i32), target.new_empty(B, dtype=torch.long),
            target.new_empty(B, dtype=torch.float32), target.new_empty(B, **i32), target.new_empty(B, **i32),
            target.new_empty(B, **i32), target.new_empty(B, **i32))


@torch.library.custom_op("specdec::verify_multi", mutates_args=())
def verify_multi(target: Tensor, draft: Tensor, draft_tokens: Tensor, stop_tokens: Tensor, kind: int,
                 temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                 row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One multi-draft verify step (ops.verify_multi): target [B, K, γ+1, V], draft [B, K, γ, V],
    draft_tokens int64 [B, K, >=γ]; the nine [B] outputs in ops.MULTI_FIELDS' order."""
    out = ops.verify_multi(target, draft, draft_tokens, _spec(kind, temperature, top_k, top_p),
                           PhiloxNoise(seed, offset), stop_tokens=stop_tokens, row_base=row_base, want_tokens=False)
    return tuple(getattr(out, f).clone() for f in ops.MULTI_FIELDS)   # views of one buffer: outputs may not alias


@verify_multi.register_fake
def _(target, draft, draft_tokens, stop_tokens, kind, temperature, top_k, top_p, seed, offset, row_base):
    B = target.shape[0]
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(target.new_empty(B, dtype=dt.get(f, torch.int32)) for f in ops.MULTI_FIELDS)


@torch.library.custom_op("specdec::verify_block", mutates_args=())
def verify_block(target: Tensor, draft: Tensor, draft_tokens: Tensor, stop_tokens: Tensor, kind: int,
                 temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                 row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One block verify step (ops.verify_block): target [B, γ+1, V], draft [B, γ, V], draft_tokens int64
    [B, >=γ]; the seven [B] outputs in ops.BLOCK_FIELDS' order, then weights [B, γ+1] and accept_prob [B, γ]."""
    out = ops.verify_block(target, draft, draft_tokens, _spec(kind, temperature, top_k, top_p),
                           PhiloxNoise(seed, offset), stop_tokens=stop_tokens, row_base=row_base, want_tokens=False)
    # views of one buffer: outputs may not alias
    return tuple(getattr(out, f).clone() for f in ops.BLOCK_FIELDS + ("weights", "accept_prob"))


@verify_block.register_fake
def _(target, draft, draft_tokens, stop_tokens, kind, temperature, top_k, top_p, seed, offset, row_base):
    B, g = target.shape[0], draft.shape[1]
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(target.new_empty(B, dtype=dt.get(f, torch.int32)) for f in ops.BLOCK_FIELDS) + (
        target.new_empty(B, g + 1, dtype=torch.float32), target.new_empty(B, g, dtype=torch.float32))


@torch.library.custom_op("specdec::verify_tree", mutates_args=())
def verify_tree(target: Tensor, draft: Tensor, draft_tokens: Tensor, parent: List[int], stop_tokens: Tensor, kind: int,
                temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One token-tree verify step (ops.verify_tree): target [B, N+1, V], draft [B, I, V] (the internal
    slots), draft_tokens int64 [B, >=N]; the seven [B] outputs in ops.TREE_FIELDS' order, then path."""
    out = ops.verify_tree(target, draft, draft_tokens, list(parent), _spec(kind, temperature, top_k, top_p),
                          PhiloxNoise(seed, offset), stop_tokens=stop_tokens, row_base=row_base, want_tokens=False)
    # views of one buffer: outputs may not alias
    return tuple(getattr(out, f).clone() for f in ops.TREE_FIELDS) + (out.path.clone(),)


@verify_tree.register_fake
def _(target, draft, draft_tokens, parent, stop_tokens, kind, temperature, top_k, top_p, seed, offset, row_base):
    from .tree import TokenTree
    B = target.shape[0]
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(target.new_empty(B, dtype=dt.get(f, torch.int32)) for f in ops.TREE_FIELDS) + (
        target.new_empty(B, TokenTree(list(parent)).depth, dtype=torch.int32),)


@torch.library.custom_op("specdec::verify_tree_distinct", mutates_args=())
def verify_tree_distinct(target: Tensor, draft_tokens: Tensor, parent: List[int], stop_tokens: Tensor, kind: int,
                         temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                         row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One token-tree verify step for distinct children (ops.verify_tree_distinct): target [B, N+1, V],
    draft_tokens int64 [B, >=N]; the seven [B] outputs in ops.TREE_FIELDS' order, then path."""
    out = ops.verify_tree_distinct(target, draft_tokens, list(parent), _spec(kind, temperature, top_k, top_p),
                                   PhiloxNoise(seed, offset), stop_tokens=stop_tokens, row_base=row_base)
    # views of one buffer: outputs may not alias
    return tuple(getattr(out, f).clone() for f in ops.TREE_FIELDS) + (out.path.clone(),)


@verify_tree_distinct.register_fake
def _(target, draft_tokens, parent, stop_tokens, kind, temperature, top_k, top_p, seed, offset, row_base):
    from .tree import TokenTree
    B = target.shape[0]
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(target.new_empty(B, dtype=dt.get(f, torch.int32)) for f in ops.TREE_FIELDS) + (
        target.new_empty(B, TokenTree(list(parent)).depth, dtype=torch.int32),)


def _pool_ns(pool_token, pool_score, pool_parent):
    from types import SimpleNamespace
    return SimpleNamespace(token=pool_token, score=pool_score, parent=pool_parent)


@torch.library.custom_op("specdec::tree_grow", mutates_args=("pool_token", "pool_score", "pool_parent"))
def tree_grow(logits: Tensor, level: int, width: int, branch: int, pool_token: Tensor, pool_score: Tensor,
              pool_parent: Tensor, frontier_in: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """One level of a dynamic draft tree (ops.tree_grow): the next frontier's tokens, pool indices and
    parent ranks, and the row status; the level's candidates are appended to the pool tensors."""
    out = ops.tree_grow(logits, level, width, branch, _pool_ns(pool_token, pool_score, pool_parent), frontier_in)
    return out.token.clone(), out.pool.clone(), out.parent_rank.clone(), out.row_status.clone()   # views of one buffer


@tree_grow.register_fake
def _(logits, level, width, branch, pool_token, pool_score, pool_parent, frontier_in=None):
    from .tree import DynamicTreeSpec
    B, Fn = logits.shape[0], DynamicTreeSpec(level, width, branch, 1).frontier[level]
    return (logits.new_empty(B, Fn, dtype=torch.long), logits.new_empty(B, Fn, dtype=torch.int32),
            logits.new_empty(B, Fn, dtype=torch.int32), logits.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("specdec::tree_select", mutates_args=())
def tree_select(pool_token: Tensor, pool_score: Tensor, pool_parent: Tensor, num_nodes: int,
                pool_size: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The rerank of a grown pool (ops.tree_select): tokens, parent, depth, pool_index, anc, row_status."""
    out = ops.tree_select(_pool_ns(pool_token, pool_score, pool_parent), num_nodes, pool_size)
    return tuple(getattr(out, f).clone() for f in ("tokens", "parent", "depth", "pool_index", "anc", "row_status"))


@tree_select.register_fake
def _(pool_token, pool_score, pool_parent, num_nodes, pool_size):
    B = pool_token.shape[0]
    e = lambda dt: pool_token.new_empty(B, num_nodes, dtype=dt)
    return (e(torch.long), e(torch.int32), e(torch.int32), e(torch.int32), e(torch.long),
            pool_token.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("specdec::verify_tree_dynamic", mutates_args=())
def verify_tree_dynamic(target: Tensor, draft_tokens: Tensor, parent_dev: Tensor, max_depth: int, stop_tokens: Tensor,
                        kind: int, temperature: float, top_k: int, top_p: float, seed: int, offset: int,
                        row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One token-tree verify step with per-sequence device topologies (ops.verify_tree_dynamic): the seven
    [B] outputs in ops.TREE_FIELDS' order, then path int32 [B, max_depth]."""
    out = ops.verify_tree_dynamic(target, draft_tokens, parent_dev, _spec(kind, temperature, top_k, top_p),
                                  PhiloxNoise(seed, offset), max_depth, stop_tokens=stop_tokens, row_base=row_base)
    return tuple(getattr(out, f).clone() for f in ops.TREE_FIELDS) + (out.path.clone(),)


@verify_tree_dynamic.register_fake
def _(target, draft_tokens, parent_dev, max_depth, stop_tokens, kind, temperature, top_k, top_p, seed, offset, row_base):
    B = target.shape[0]
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(target.new_empty(B, dtype=dt.get(f, torch.int32)) for f in ops.TREE_FIELDS) + (
        target.new_empty(B, max_depth, dtype=torch.int32),)


def _vp_step(target: Tensor, draft: Tensor, draft_tokens: Tensor, stop_tokens, shard: int, num_shards: int,
             vocab_offset: int, vocab: int, kind: int, temperature: float, skip: bool, seed: int, offset: int,
             row_base: int) -> vp._Step:
    sh = vp.VocabShard(shard, num_shards, vocab_offset, target.shape[-1], vocab)
    nz, _ = ops._noise_struct(PhiloxNoise(seed, offset), 0, target.device, row_base)
    return vp._step_of(target, draft if draft.shape[1] else None, draft_tokens, vp._vp_spec(_spec(kind, temperature, 0, 1.0)),
                       nz, sh, stop_tokens, skip)


@torch.library.custom_op("specdec::vp_stats", mutates_args=())
def vp_stats(target: Tensor, draft: Tensor, draft_tokens: Tensor, shard: int, num_shards: int, vocab_offset: int,
             vocab: int, kind: int, temperature: float) -> Tensor:
    """Phase 1 of the vocabulary-parallel verify on this rank's slices: its statistics block."""
    return _vp_step(target, draft, draft_tokens, None, shard, num_shards, vocab_offset, vocab, kind, temperature, False,
                    0, 0, 0).stats()


@vp_stats.register_fake
def _(target, draft, draft_tokens, shard, num_shards, vocab_offset, vocab, kind, temperature):
    B, g = target.shape[0], target.shape[1] - 1
    return target.new_empty(32 + B * (2 * g + 1) * 16, dtype=torch.uint8)


@torch.library.custom_op("specdec::vp_decide", mutates_args=())
def vp_decide(target: Tensor, draft: Tensor, draft_tokens: Tensor, stop_tokens: Tensor, stats_all: Tensor, shard: int,
              num_shards: int, vocab_offset: int, vocab: int, kind: int, temperature: float,
              skip_sample_adjustment: bool, seed: int, offset: int, row_base: int) -> Tensor:
    """Phase 3: the decision (the same on every rank) and this rank's candidate block."""
    return _vp_step(target, draft, draft_tokens, stop_tokens, shard, num_shards, vocab_offset, vocab, kind, temperature,
                    skip_sample_adjustment, seed, offset, row_base).decide(stats_all)


@vp_decide.register_fake
def _(target, draft, draft_tokens, stop_tokens, stats_all, shard, num_shards, vocab_offset, vocab, kind, temperature,
      skip_sample_adjustment, seed, offset, row_base):
    return target.new_empty(32 + target.shape[0] * 32, dtype=torch.uint8)


@torch.library.custom_op("specdec::vp_finish", mutates_args=())
def vp_finish(cand_all: Tensor, gamma: int, shard: int, num_shards: int, vocab_offset: int, vocab_local: int,
              vocab: int, kind: int, seed: int, offset: int,
              row_base: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Phase 5: the shard pick and the step's outputs, in vocab_parallel.VP_FIELDS' order."""
    B = (cand_all.shape[1] - 32) // 32
    sh = vp.VocabShard(shard, num_shards, vocab_offset, vocab_local, vocab)
    nz, _ = ops._noise_struct(PhiloxNoise(seed, offset), 0, cand_all.device, row_base)
    st = vp._Step(B, gamma, cand_all.device, torch.float32, sh, vp._vp_spec(_spec(kind, 1.0, 0, 1.0)), nz)
    out = st.finish(cand_all)
    return tuple(getattr(out, f).clone() for f in vp.VP_FIELDS)   # views of one buffer: outputs may not alias


@vp_finish.register_fake
def _(cand_all, gamma, shard, num_shards, vocab_offset, vocab_local, vocab, kind, seed, offset, row_base):
    B = (cand_all.shape[1] - 32) // 32
    dt = {"next_token": torch.long, "resample_mass": torch.float32}
    return tuple(cand_all.new_empty(B, dtype=dt.get(f, torch.int32)) for f in vp.VP_FIELDS)


@torch.library.custom_op("specdec::beam_topk", mutates_args=())
def beam_topk(logits: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """topk(log_softmax(logits [R, V], -1), k) in one pass over the rows (sampling/base_decoding.py:
    136-137): (logprob fp32 [R, k] holding the value rounded to the logits dtype, token int64 [R, k]),
    value descending, lowest index first among equal values."""
    return ops.beam_topk(logits, k)


@beam_topk.register_fake
def _(logits, k):
    R = logits.shape[0]
    return logits.new_empty(R, k, dtype=torch.float32), logits.new_empty(R, k, dtype=torch.long)


@torch.library.custom_op("specdec::kv_compact", mutates_args=("tensors",))
def kv_compact(tensors: List[Tensor], path: Tensor, count: Tensor, base: int, num_slots: int,
               node_slot: Optional[List[int]] = None, base_dev: Optional[Tensor] = None) -> None:
    """ops.kv_compact: the K/V tensors of all layers compacted in place onto verify_tree's path."""
    ops.kv_compact(tensors, path, count, base, num_slots=num_slots, node_slot=node_slot, base_dev=base_dev)


@kv_compact.register_fake
def _(tensors, path, count, base, num_slots, node_slot=None, base_dev=None):
    return None
