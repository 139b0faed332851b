"""GPU tests of sd_kv_compact_ragged (ops.kv_compact with one base per sequence, csrc/kv_compact.hip): bit
for bit against the host model (tests/kv_ref.py) applied to every sequence with its own base, on a buffer
of random 16-bit words (the poison) that must equal the host model's everywhere afterwards."""
import pytest
import torch

import kv_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD = 0x40                                   # SD_ROW_INVALID_DIST
H, L, SLOTS = 2, 40, 10
PATH = [[1, 4, 8], [0, 3, 7], [1, 5, 9], [0, 2, 6]]


def _tensors(buf, B, D):
    """Two [B, H, L, D] bf16 views into the int16 buffer, 64 words of guard around each."""
    n = B * H * L * D
    return [buf[at:at + n].view(torch.bfloat16).view(B, H, L, D) for at in (64, 64 + n + 64)]


@pytest.mark.parametrize("D", [8, 5], ids=["16-byte-rows", "10-byte-rows"])
@pytest.mark.parametrize("bases, flagged", [((0, 5, L - SLOTS), False), ((0, 5, L - SLOTS, L - SLOTS + 1), True),
                                            ((3, -1, 7), True)])
def test_every_sequence_moves_from_its_own_base(bases, flagged, D):
    from specdec_amd import ops
    B = len(bases)
    host = torch.randint(-32768, 32767, (2 * (B * H * L * D + 64) + 64,), dtype=torch.int16,
                         generator=torch.Generator().manual_seed(B))
    dev = host.to(DEV)
    path, count = torch.tensor(PATH[:B], dtype=torch.int32), torch.full((B,), 3, dtype=torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_compact(_tensors(dev, B, D), path.to(DEV), count.to(DEV), 0, num_slots=SLOTS, status_or=status,
                   base_dev=torch.tensor(bases, dtype=torch.long, device=DEV))
    for b, base in enumerate(bases):
        if 0 <= base <= L - SLOTS:           # a base that leaves the buffer moves nothing
            assert not kv_ref.compact([t[b:b + 1] for t in _tensors(host, B, D)], path[b:b + 1], count[b:b + 1], base, SLOTS)
    assert torch.equal(dev.cpu(), host)
    assert int(status.item()) == (BAD if flagged else 0)


def test_one_element_at_batch_one_is_the_shared_base_call():
    from specdec_amd import ops
    host = torch.randint(-32768, 32767, (2 * (H * L * 8 + 64) + 64,), dtype=torch.int16, generator=torch.Generator().manual_seed(7))
    got, want = host.to(DEV), host.to(DEV)
    path = torch.tensor(PATH[:1], dtype=torch.int32, device=DEV)
    count = torch.tensor([3], dtype=torch.int32, device=DEV)
    ops.kv_compact(_tensors(got, 1, 8), path, count, 2, num_slots=SLOTS, base_dev=torch.tensor([9], dtype=torch.long, device=DEV))
    ops.kv_compact(_tensors(want, 1, 8), path, count, 11, num_slots=SLOTS)
    assert torch.equal(got, want) and not torch.equal(got.cpu(), host)
