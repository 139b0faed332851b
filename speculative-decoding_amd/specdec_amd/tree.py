"""Token trees for tree speculative decoding (sd_verify_tree).

A tree of N drafted nodes hangs below the last committed token (the root).  Nodes are numbered
0..N-1 with ``parent[i]`` in {-1, 0..i-1} (-1: a child of the root); slot 0 is the root and slot
i + 1 is node i.  The limits are the C side's: N <= 64, at most 8 children per slot, depth <= 32.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

MAX_NODES, MAX_CHILDREN, MAX_DEPTH = 64, 8, 32      # SD_TREE_MAX_NODES, SD_TREE_MAX_CHILDREN, SD_MAX_GAMMA
MAX_WIDTH, MAX_POOL = 8, 2048                       # SD_TREE_GROW_MAX_WIDTH, SD_TREE_POOL_MAX


class TokenTree:
    """One topology: ``parent`` (validated as sd_verify_tree validates it) and what follows from it.

    depth            the longest root-to-leaf path, in nodes
    node_depth[i]    depth of node i (children of the root: 1)
    children[s]      nodes below slot s, ascending
    internal_slots   slots with children, ascending (the rows a drafter must provide)
    levels[d]        nodes of depth d + 1, ascending
    """

    def __init__(self, parent: Sequence[int]):
        parent = [int(p) for p in parent]
        n = len(parent)
        if n == 0:
            raise ValueError("a token tree needs at least one node")
        if n > MAX_NODES:
            raise ValueError(f"a token tree has at most {MAX_NODES} nodes, got {n}")
        for i, p in enumerate(parent):
            if not -1 <= p < i:
                raise ValueError(f"parent[{i}] = {p}: a node's parent is -1 (the root) or a node below its index")
        self.parent: List[int] = parent
        self.num_nodes = n
        self.children: List[List[int]] = [[] for _ in range(n + 1)]
        self.node_depth: List[int] = []
        for i, p in enumerate(parent):
            self.children[p + 1].append(i)
            self.node_depth.append(1 if p < 0 else self.node_depth[p] + 1)
        self.depth = max(self.node_depth)
        self.max_children = max(len(c) for c in self.children)
        if self.max_children > MAX_CHILDREN:
            raise ValueError(f"a slot has at most {MAX_CHILDREN} children, got {self.max_children}")
        if self.depth > MAX_DEPTH:
            raise ValueError(f"a token tree is at most {MAX_DEPTH} deep, got {self.depth}")
        self.internal_slots: List[int] = [s for s, c in enumerate(self.children) if c]
        self.levels: List[List[int]] = [[i for i in range(n) if self.node_depth[i] == d + 1] for d in range(self.depth)]

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_branching(cls, branching: Sequence[int]) -> "TokenTree":
        """The full tree with branching[d] children under every node of depth d (the root: depth 0),
        numbered level by level."""
        parent: List[int] = []
        level = [-1]
        for width in branching:
            if width < 1:
                raise ValueError("every branching factor is at least 1")
            nxt = []
            for p in level:
                for _ in range(int(width)):
                    nxt.append(len(parent))
                    parent.append(p)
            level = nxt
        return cls(parent)

    @classmethod
    def chains(cls, num_chains: int, gamma: int) -> "TokenTree":
        """K independent chains of γ nodes: node d*K + k is chain k's depth-d draft (parent i - K)."""
        if num_chains < 1 or gamma < 1:
            raise ValueError("chains needs num_chains >= 1 and gamma >= 1")
        return cls([i - num_chains if i >= num_chains else -1 for i in range(num_chains * gamma)])

    # ------------------------------------------------------------------ derived
    def truncated(self, depth: int) -> "TokenTree":
        """The nodes of depth <= `depth`, renumbered in order (for the end of a sequence)."""
        if depth >= self.depth:
            return self
        keep = [i for i in range(self.num_nodes) if self.node_depth[i] <= depth]
        if not keep:
            raise ValueError("truncated: depth must be at least 1")
        new = {i: j for j, i in enumerate(keep)}
        return TokenTree([new[self.parent[i]] if self.parent[i] >= 0 else -1 for i in keep])

    def path_to(self, node: int) -> List[int]:
        """The nodes from the root's child down to `node`."""
        out = []
        while node >= 0:
            out.append(node)
            node = self.parent[node]
        return out[::-1]

    def ancestor_matrix(self) -> torch.Tensor:
        """bool [N, N]: entry (i, j) says node j is node i or one of its ancestors."""
        n = self.num_nodes
        m = torch.zeros(n, n, dtype=torch.bool)
        for i in range(n):
            m[i, self.path_to(i)] = True
        return m

    def attention_inputs(self, prefix_len: int, dtype: torch.dtype = torch.float32, device=None, num_nodes=None):
        """(mask, position_ids) of a forward over prefix + the first `num_nodes` nodes (default: all):
        the 4-D additive mask [1, 1, L, L] (0 where attention is allowed, finfo(dtype).min where not)
        and position_ids [1, L], L = prefix_len + nodes.  The prefix is causal; node i sees the prefix,
        its ancestors and itself, and sits at position prefix_len + depth(i) - 1."""
        n = self.num_nodes if num_nodes is None else int(num_nodes)
        L = prefix_len + n
        allow = torch.zeros(L, L, dtype=torch.bool)
        allow[:prefix_len, :prefix_len] = torch.ones(prefix_len, prefix_len, dtype=torch.bool).tril()
        allow[prefix_len:, :prefix_len] = True
        allow[prefix_len:, prefix_len:] = self.ancestor_matrix()[:n, :n]
        mask = torch.zeros(L, L, dtype=dtype)
        mask.masked_fill_(~allow, torch.finfo(dtype).min)
        pos = torch.cat([torch.arange(prefix_len), torch.tensor([prefix_len + d - 1 for d in self.node_depth[:n]],
                                                                 dtype=torch.long)])
        return mask[None, None].to(device), pos[None].to(device)

    def __repr__(self) -> str:
        return f"TokenTree(nodes={self.num_nodes}, depth={self.depth}, parent={self.parent})"


class DynamicTreeSpec:
    """The static shape of a dynamic draft tree (sd_tree_grow / sd_tree_select): ``levels``
    growth levels, ``width`` frontier nodes expanded per level, ``branch`` children per expanded node and
    ``num_nodes`` nodes sent to the target.  What the host knows without reading a score:

    frontier[l]   nodes of the frontier after level l (frontier[0] = 1, the root): min(width, frontier[l-1] * branch)
    base[l]       pool index of level l + 1's first candidate; level l + 1 adds frontier[l] * branch
    pool_size     base[levels]
    """

    def __init__(self, levels: int, width: int, branch: int, num_nodes: int):
        levels, width, branch, num_nodes = int(levels), int(width), int(branch), int(num_nodes)
        if not 1 <= levels <= MAX_DEPTH:
            raise ValueError(f"levels must be in 1..{MAX_DEPTH}, got {levels}")
        if not 1 <= width <= MAX_WIDTH:
            raise ValueError(f"width must be in 1..{MAX_WIDTH}, got {width}")
        if not 1 <= branch <= MAX_CHILDREN:
            raise ValueError(f"branch must be in 1..{MAX_CHILDREN}, got {branch}")
        self.levels, self.width, self.branch = levels, width, branch
        self.frontier: List[int] = [1]
        self.base: List[int] = [0]
        for _ in range(levels):
            self.base.append(self.base[-1] + self.frontier[-1] * branch)
            self.frontier.append(min(width, self.frontier[-1] * branch))
        self.pool_size = self.base[-1]
        if self.pool_size > MAX_POOL:
            raise ValueError(f"the pool holds at most {MAX_POOL} candidates, this shape makes {self.pool_size}")
        if not 1 <= num_nodes <= min(MAX_NODES, self.pool_size):
            raise ValueError(f"num_nodes must be in 1..{min(MAX_NODES, self.pool_size)}, got {num_nodes}")
        self.num_nodes = num_nodes

    def truncated(self, depth: int) -> "DynamicTreeSpec":
        """The first `depth` levels, num_nodes cut to the smaller pool (for the end of a sequence)."""
        if depth >= self.levels:
            return self
        if depth < 1:
            raise ValueError("truncated: depth must be at least 1")
        pool = self.base[depth]
        return DynamicTreeSpec(depth, self.width, self.branch, min(self.num_nodes, pool))

    def __repr__(self) -> str:
        return (f"DynamicTreeSpec(levels={self.levels}, width={self.width}, branch={self.branch}, "
                f"num_nodes={self.num_nodes}, pool={self.pool_size})")


def dynamic_attention_inputs(anc: torch.Tensor, depth: torch.Tensor, prefix_len: int, dtype: torch.dtype = torch.float32):
    """(mask, position_ids) of a forward over prefix + the N nodes ``tree_select`` chose, built on the
    device from its ``anc`` int64 [B, N] and ``depth`` int32 [B, N] with ``TokenTree.attention_inputs``'
    conventions: the additive mask [B, 1, L, L] (0 where attention is allowed, finfo(dtype).min where
    not), L = prefix_len + N, and position_ids [B, L] with node i at prefix_len + depth(i) - 1.  No host
    read."""
    B, n = anc.shape
    dev = anc.device
    L = prefix_len + n
    allow = torch.zeros(B, L, L, dtype=torch.bool, device=dev)
    allow[:, :prefix_len, :prefix_len] = torch.ones(prefix_len, prefix_len, dtype=torch.bool, device=dev).tril()
    allow[:, prefix_len:, :prefix_len] = True
    bits = torch.arange(n, device=dev, dtype=torch.long)
    allow[:, prefix_len:, prefix_len:] = ((anc[:, :, None] >> bits[None, None, :]) & 1).bool()
    mask = torch.zeros(B, L, L, dtype=dtype, device=dev)
    mask.masked_fill_(~allow, torch.finfo(dtype).min)
    pos = torch.cat([torch.arange(prefix_len, device=dev).expand(B, prefix_len), prefix_len + depth.long() - 1], 1)
    return mask[:, None], pos
