"""CPU restatement of the beam-search loop (sampling/base_decoding.py:68-187) that the device beam
step (csrc/beam.hip) is checked against, in the style of tests/philox_ref.py.

Two things are written out explicitly instead of being left to torch:

* top-k ties: equal values are ordered lowest index first (``torch.topk`` leaves the order
  undefined);
* the reference's update of ``beams_probs`` / ``last_indexes``: a finished beam's candidate holds
  0-dim VIEWS of its old slot, and the slots are rewritten in beam order, so a finished beam that
  sorts to a higher slot takes whatever its old slot holds by then (``copy_semantics=True`` gives the
  variant with copies, which is NOT what the reference returns).

Log-probs of 16-bit rows are fp32 inside and rounded once (see ``logprob_topk``).  Scores are fp32:
one add and one IEEE division per candidate, done here in numpy float32.
"""
from __future__ import annotations

import numpy as np
import torch

F32_MIN = float(torch.finfo(torch.float).min)


def length_penalty(length, alpha, min_length) -> np.float32:
    lp = ((min_length + length) / (min_length + 1)) ** alpha
    return np.float32(lp if lp != 0 else 1)


def topk_lowest_index(values: torch.Tensor, k: int):
    """(values, indices) of the k largest along the last axis, value descending, index ascending."""
    v, i = torch.sort(values, dim=-1, descending=True, stable=True)
    return v[..., :k].contiguous(), i[..., :k].contiguous()


def logprob_topk(logits: torch.Tensor, k: int):
    """topk(log_softmax(logits), k) in the logits dtype: (fp32 values holding the rounded log-probs,
    int64 ids), lowest index first among equal values.  The log-softmax is fp32 inside and rounded
    ONCE to a 16-bit dtype, as torch computes it on a GPU and as the kernel does.  torch's CPU
    kernel for 16-bit rows also rounds the row's sum and its logarithm to the dtype, which moves
    about one log-prob in four by a step of the dtype; the reference's CPU goldens carry that."""
    lp = torch.nn.functional.log_softmax(logits.float(), dim=-1).to(logits.dtype)
    v, i = topk_lowest_index(lp, k)
    return v.float(), i


def initial_state(inputs, num_beams, total_len, pad):
    P = len(inputs)
    ids = torch.full((num_beams, total_len), pad, dtype=torch.long)
    ids[:, :P] = torch.tensor(inputs, dtype=torch.long)
    probs = torch.full((num_beams, total_len), F32_MIN, dtype=torch.float)
    probs[:, :P] = 1.0
    return dict(ids=ids, probs=probs, bp=torch.full((num_beams,), 1.0), li=torch.full((num_beams,), -1, dtype=torch.long))


def prefill(state, top_lp, top_tok, P, lp):
    """:129-131 — top_lp / top_tok: [1, num_beams]."""
    ids, probs = state["ids"].clone(), state["probs"].clone()
    n = ids.shape[0]
    newp = (probs[:, P - 1].numpy() + top_lp[0].numpy().astype(np.float32)).astype(np.float32)
    ids[:, P] = top_tok[0]
    probs[:, P] = torch.from_numpy(newp)
    bp = torch.from_numpy((newp / np.float32(lp)).astype(np.float32))
    parent = torch.tensor([[b, b] for b in range(n)], dtype=torch.int32)
    return dict(ids=ids, probs=probs, bp=bp, li=state["li"].clone(), parent=parent,
                all_finished=int(bool((state["li"] != -1).all())))


def select(state, top_lp, top_tok, curr, lp, stops, pad, copy_semantics=False, info=None):
    """:138-180 for one step.  top_lp fp32 [n, k], top_tok int64 [n, k].  Returns the new state with
    ``parent`` (source beam, candidate index or -1) and ``all_finished`` (-1: fewer candidates than
    beams, where the reference raises IndexError)."""
    ids, probs, bp, li = state["ids"], state["probs"], state["bp"], state["li"]
    n, k = top_lp.shape
    lp32 = np.float32(lp)
    stops = set(int(s) for s in stops)
    ent = []   # (score, ids row, probs row, fresh last index or None, finished-from slot or None, (src, j))
    for b in range(n):
        if int(li[b]) != -1:
            ent.append((np.float32(bp[b].item()), ids[b].clone(), probs[b].clone(), None, b, (b, -1)))
            continue
        for j in range(k):
            newp = np.float32(np.float32(probs[b, curr - 1].item()) + np.float32(top_lp[b, j].item()))
            tok = int(top_tok[b, j])
            row = ids[b].clone()
            row[curr] = tok
            if any(torch.equal(e[1], row) for e in ent):
                continue
            prow = probs[b].clone()
            prow[curr] = float(newp)
            last = curr if (tok in stops or tok == pad) else -1
            ent.append((np.float32(newp / lp32), row, prow, last, None, (b, j)))
    order = sorted(range(len(ent)), key=lambda e: -float(ent[e][0]))   # stable: equal scores keep their order
    if info is not None:
        sc = sorted((float(e[0]) for e in ent), reverse=True)[:n + 1]
        gaps = [a - b for a, b in zip(sc, sc[1:])]
        info["score_gap"] = min([g for g in gaps if g > 0], default=float("inf"))
        info["score_ties"] = sum(1 for g in gaps if g == 0)
    if len(order) < n:
        return dict(ids=ids.clone(), probs=probs.clone(), bp=bp.clone(), li=li.clone(),
                    parent=torch.full((n, 2), -1, dtype=torch.int32), all_finished=-1)
    out_ids, out_probs = ids.clone(), probs.clone()
    out_bp, out_li = bp.clone(), li.clone()
    old_bp, old_li = bp.clone(), li.clone()
    parent = torch.zeros(n, 2, dtype=torch.int32)
    for b in range(n):   # in beam order; a view reads the slot's CURRENT value
        score, row, prow, last, slot, par = ent[order[b]]
        out_ids[b], out_probs[b] = row, prow
        if slot is None:
            out_bp[b], out_li[b] = float(score), last
        elif copy_semantics:
            out_bp[b], out_li[b] = old_bp[slot], old_li[slot]
        else:
            out_bp[b], out_li[b] = out_bp[slot].clone(), out_li[slot].clone()
        parent[b, 0], parent[b, 1] = par
    return dict(ids=out_ids, probs=out_probs, bp=out_bp, li=out_li, parent=parent,
                all_finished=int(bool((out_li != -1).all())))


def bits(t: torch.Tensor):
    return t.contiguous().view(torch.int32).tolist()


@torch.no_grad()
def beam_search(inputs, model, max_gen_len=40, num_beams=4, top_k=3, min_length=5.0, alpha=1.2, eos_tokens_id=1,
                pad_token_id=0, copy_semantics=False, trace=None, topk_fn=logprob_topk):
    """The whole loop.  trace (a list): one dict per model call after the first — the state that call
    sees (``bp`` bit patterns, ``li``) — plus, when the call is followed by a step, the step's info."""
    P = len(inputs)
    cfg = model.config
    max_seq = cfg.max_position_embeddings if hasattr(cfg, "max_position_embeddings") else 1024
    total_len = min(max_seq, P + max_gen_len)
    if total_len <= P:
        raise IndexError(f"index {P} is out of bounds for dimension 1 with size {total_len}")
    stops = eos_tokens_id if isinstance(eos_tokens_id, list) else [eos_tokens_id]
    st = initial_state(inputs, num_beams, total_len, pad_token_id)
    o = model(st["ids"][:, :P])
    st = prefill(st, *topk_fn(o.logits[0:1, -1, :], num_beams), P, length_penalty(1, alpha, min_length))
    for curr in range(P + 1, total_len):
        if trace is not None:
            trace.append(dict(bp=bits(st["bp"]), li=st["li"].tolist()))
        o = model(st["ids"][:, :curr])
        tl, tt = topk_fn(o.logits[:, -1, :], top_k)
        info = {} if trace is not None else None
        new = select(st, tl, tt, curr, length_penalty(curr - P, alpha, min_length), stops, pad_token_id,
                     copy_semantics, info)
        if trace is not None:
            other = select(st, tl, tt, curr, length_penalty(curr - P, alpha, min_length), stops, pad_token_id,
                           not copy_semantics)
            info["aliasing"] = not (torch.equal(other["bp"], new["bp"]) and torch.equal(other["li"], new["li"]))
            info["carried"] = int(((st["li"] != -1).sum() > 0) and ((st["li"] == -1).sum() > 0))
            trace[-1].update(info)
        st = new
        if st["all_finished"] < 0:
            raise IndexError("list index out of range")
        if st["all_finished"]:
            break
    li = st["li"].clone()
    li[li == -1] = total_len - 1
    return st["ids"][0, P:int(li[0]) + 1].tolist()
