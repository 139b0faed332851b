"""Without-replacement token trees on the host: the rule is lossless by exact enumeration, the ABI
additions move no struct, and the GPU grids' close-call caps hold for the host model (their case builders run here)."""
import ctypes as C
import functools

import numpy as np
import pytest

import tree_swor_ref as sw
import tree_walk as tw

V = 4


def _row(salt, prefix):                                # context-dependent probabilities
    w = np.random.default_rng([salt, len(prefix), *prefix]).random(V) ** 2 + 0.02
    return w / w.sum()


@pytest.mark.parametrize("parent,forced", [(tw.from_branching([3]), ()), (tw.from_branching([2, 2]), ()),
                                           ([-1, -1, 0, 0, 1], (3,))], ids=["b3", "b22", "irregular-1"])
def test_first_two_tokens_keep_the_targets_joint(parent, forced):
    p_of = functools.partial(_row, 1)
    joint = sw.enumerate_joint(p_of, functools.partial(_row, 2), V, parent, forced)
    want = np.array([[p_of(())[a] * p_of((a,))[b] for b in range(V)] for a in range(V)])
    assert np.abs(joint - want).max() < 1e-12


def test_abi_additions_move_no_struct():
    from specdec_amd import _lib
    assert C.sizeof(_lib.sd_tree_args) == 1560 and _lib.sd_tree_args.status_or.offset == 1552
    a = _lib.sd_sample_distinct_args
    assert (a.logits.offset, a.proc.offset, a.noise.offset, a.tokens.offset, a.workspace_bytes.offset) == (16, 32, 48, 104, 152)
    assert _lib.SD_PATH_VERIFY_TREE_SWOR == 12 and _lib.SD_PATH_SAMPLE_DISTINCT == 22
    assert {"sd_sample_distinct", "sd_verify_tree_swor"} <= set(_lib.EXPORTS)


def test_gpu_grids_have_no_close_calls():
    import test_gpu_sample_distinct as gd
    import test_gpu_tree_swor as gs
    for case in gd.CASES:
        assert gd.host(*case).close == 0, case          # the seed is chosen so that no rank is close
    for case in gs.WALKS:
        assert sum(r.close for r in gs.host_walk(*case)[1]) <= 1, case
