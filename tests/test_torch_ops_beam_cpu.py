"""torch.ops.specdec.beam_topk is registered and its fake implementation gives the output shapes and
dtypes without a GPU (meta tensors)."""
import pytest
import torch

import specdec_amd  # noqa: F401  (registers the ops)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_beam_topk_op_fake_shapes(dtype):
    x = torch.empty(4, 128256, device="meta", dtype=dtype)
    lp, tok = torch.ops.specdec.beam_topk(x, 3)
    assert (lp.shape, lp.dtype, lp.device.type) == ((4, 3), torch.float32, "meta")
    assert (tok.shape, tok.dtype, tok.device.type) == ((4, 3), torch.long, "meta")
    lp, tok = torch.ops.specdec.beam_topk(x[:1], 64)
    assert lp.shape == (1, 64) and tok.shape == (1, 64)
