"""CPU: the host side of `_packed_files`, which needs neither the library nor a GPU: the staging rule of `pack` (every item at a
multiple of 16 bytes, zeros between them) and the descriptor rows `descriptor_rows` hands to the decode kernels."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import _packed_files as P
from dad_3dheads_amd.dataset import FileBatchCollate


def test_pack_puts_every_item_at_a_multiple_of_16_with_zeros_between():
    rng = np.random.default_rng(3)
    items = [rng.integers(1, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 15, 16, 17, 33)]  # no zero byte inside an item
    buffer, table = P.pack(items)
    assert buffer.dtype == torch.uint8 and buffer.device.type == "cpu" and not buffer.is_pinned() and buffer.numel() == 128
    assert table.dtype == np.int64 and table[:, 0].tolist() == [0, 0, 16, 32, 48, 80] and table[:, 1].tolist() == [0, 1, 15, 16, 17, 33]
    flat, inside = buffer.numpy(), np.zeros(128, dtype=bool)
    for (off, size), item in zip(table.tolist(), items):
        assert flat[off:off + size].tobytes() == item
        inside[off:off + size] = True
    assert not flat[~inside].any() and flat[inside].all()
    arrays = [np.frombuffer(b, dtype=np.uint8) for b in items]
    packed, collate_table = FileBatchCollate._pack(arrays)  # the collate's packer is this one
    assert torch.equal(packed, buffer) and np.array_equal(collate_table, table) and not packed.is_pinned()
    assert [P.align(n) for n in (0, 1, 15, 16, 17, 33)] == [0, 16, 16, 16, 32, 48] and P.ALIGN == 16
    empty, none = P.pack([])
    assert empty.numel() == 0 and none.shape == (0, 2)
    least, _ = P.pack([b"ab"], min_bytes=48)
    assert least.numel() == 48 and least[:3].tolist() == [97, 98, 0]


def test_check_packed_refuses_what_breaks_the_contract():
    buffer = torch.zeros(64, dtype=torch.uint8)
    assert P.check_packed(buffer, np.array([0, 32]), np.array([20, 32]), [None, (1, 1, 1)]) == ([0, 32], [20, 32])
    assert P.check_packed(buffer, [8], [0], None) == ([8], [0])  # a file of no bytes lies nowhere
    for bad in (lambda: P.check_packed(buffer, [8], [20], None), lambda: P.check_packed(buffer, [32], [33], None),
                lambda: P.check_packed(buffer, [0, 16], [20], None), lambda: P.check_packed(buffer, [-16], [20], None),
                lambda: P.check_packed(buffer, [0], [-1], None), lambda: P.check_packed(buffer.to(torch.int8), [0], [20], None),
                lambda: P.check_packed(buffer.view(2, -1), [0], [20], None), lambda: P.check_packed(buffer[::2], [0], [20], None),
                lambda: P.check_packed(buffer.numpy(), [0], [20], None), lambda: P.check_packed(buffer, [0], [20], [])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="multiple of 16"):
        P.check_packed(buffer, [8], [20], None)


def test_descriptor_rows_and_output_size():
    heads, sizes, offsets = [(5, 7, 3), None, (8, 8, 1)], [100, 40, 0], [0, 112, 160]
    on_device = P.on_device(sizes, heads)
    assert on_device == [0]  # item 1 has no head, item 2 no bytes
    for channels in (None, 3):
        rows, out_bytes = P.descriptor_rows(offsets, sizes, heads, channels, on_device)
        assert rows == [[0, 100, 5, 7, 3, 0, 21, 3, 0, 0, 0, 0]] and out_bytes == 112  # 5 * 7 * 3 = 105, rounded up to 16
    rows, out_bytes = P.descriptor_rows(offsets, sizes, heads, 1, [0, 2])  # as if item 2 held bytes: the second output behind the first
    assert rows == [[0, 100, 5, 7, 3, 0, 7, 1, 0, 0, 0, 0], [160, 0, 8, 8, 1, 48, 8, 1, 0, 0, 0, 0]] and out_bytes == 48 + 64
