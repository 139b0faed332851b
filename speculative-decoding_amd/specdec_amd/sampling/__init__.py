from .base_decoding import autoregressive_generate, beam_search_generate  # noqa: F401
from .speculative_decoding import max_fn, speculative_generate  # noqa: F401
from .multidraft_decoding import multidraft_speculative_generate  # noqa: F401
from .block_decoding import block_speculative_generate  # noqa: F401
from .tree_decoding import tree_speculative_generate  # noqa: F401
from .dynamic_tree_decoding import dynamic_tree_speculative_generate  # noqa: F401
from .vocab_parallel_decoding import vocab_parallel_speculative_generate  # noqa: F401
