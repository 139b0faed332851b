"""specdec_amd — MI355X-native speculative verify/accept path (drop-in for the hot path of
dadiaokua/speculative-decoding).

Module layout mirrors the reference's import paths for the hot path:

    specdec_amd.utils.logits_processor   <- utils/logits_processor.py
    specdec_amd.utils.caching            <- utils/caching.py; compact_cache (a cache onto a tree's accepted path)
    specdec_amd.sampling                 <- sampling/speculative_decoding.py (speculative_generate, max_fn);
                                            multidraft_speculative_generate (K draft chains per step);
                                            block_speculative_generate (the drafted block verified jointly);
                                            vocab_parallel_speculative_generate (tensor-parallel target);
                                            dynamic_tree_speculative_generate (device-grown draft trees)
    specdec_amd.vocab_parallel           verify on vocabulary slices (VocabShard, verify_vocab_parallel,
                                            GroupExchange, LocalShards)
    specdec_amd.engine.infer_engine      <- engine/infer_engine.py (infer_batch, run_batch_speculative,
                                            batch_speculative_generate)
    specdec_amd.engine.metrics           <- engine/metrics.py (the bookkeeping dataclasses it feeds)

All compute goes through libspecdec.so (HIP, gfx950); importing fails if it is missing.
"""
from . import _lib  # noqa: F401  (loads libspecdec.so or raises)
from ._lib import RowError, get_poll_policy, set_poll_policy  # noqa: F401
from .noise import PhiloxNoise, StreamNoise, default_noise, set_noise_mode  # noqa: F401
from .ops import ProcSpec, kv_compact, proc_spec, probs_rows, sample_rows, verify, verify_multi, verify_tree  # noqa: F401
from .ops import topk_children, verify_tree_distinct  # noqa: F401
from .ops import BlockVerifyOut, verify_block  # noqa: F401
from .ops import tree_grow, tree_pool, tree_select, verify_tree_dynamic  # noqa: F401
from .tree import DynamicTreeSpec, TokenTree, dynamic_attention_inputs  # noqa: F401
from .vocab_parallel import GroupExchange, LocalShards, VocabShard, verify_vocab_parallel  # noqa: F401
from . import torch_ops  # noqa: F401,E402  (registers torch.ops.specdec.sample / .verify)
from .sampling.dynamic_tree_decoding import dynamic_tree_speculative_generate  # noqa: F401,E402

__all__ = ["RowError", "get_poll_policy", "set_poll_policy", "PhiloxNoise", "StreamNoise", "default_noise", "set_noise_mode", "ProcSpec", "proc_spec",
           "probs_rows", "sample_rows", "verify", "verify_multi", "verify_block", "verify_tree", "verify_tree_distinct", "topk_children", "kv_compact", "TokenTree", "GroupExchange", "LocalShards", "VocabShard",
           "verify_vocab_parallel", "tree_grow", "tree_pool", "tree_select", "verify_tree_dynamic", "DynamicTreeSpec",
           "dynamic_attention_inputs", "dynamic_tree_speculative_generate"]
