"""CPU: the host side of the frames chain. `frame_table` reads tensor metadata only, so it is checked on CPU tensors; and the
painter's-order reading of the reference -- a loop over `rasterize(.., bg=frame)` gives every head a z-buffer of its own, so the head
drawn second wins where it covers, also where it lies behind -- is pinned on the compiled reference (the C port where it is absent)."""
import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib
from dad_3dheads_amd.Sim3DR.frames import frame_table
from render_frames_restatement import expected_frames


def test_frame_table_of_a_contiguous_frame_a_view_and_a_batch():
    a = torch.zeros((96, 160, 3), dtype=torch.uint8)
    wide = torch.zeros((130, 80, 3), dtype=torch.uint8)
    view = wide[:, 5:75]
    table, shapes = frame_table([a, view])
    assert table.dtype == np.int64 and table.shape == (2, 4) and shapes == [(96, 160), (130, 70)]
    assert table[0].tolist() == [a.data_ptr(), 96, 160, 480]
    assert table[1].tolist() == [wide.data_ptr() + 15, 130, 70, 240]  # an odd address and a stride that is not 3 * w
    batch = torch.zeros((3, 64, 64, 3), dtype=torch.uint8)
    table, shapes = frame_table(batch)
    assert shapes == [(64, 64)] * 3
    assert table.tolist() == [[batch.data_ptr() + i * 64 * 64 * 3, 64, 64, 192] for i in range(3)]
    row = torch.zeros((1, 10, 3), dtype=torch.uint8)
    assert frame_table([row])[0][0].tolist() == [row.data_ptr(), 1, 10, 30]
    table, shapes = frame_table([])
    assert table.shape == (0, 4) and shapes == []


def test_frame_table_refuses_what_the_kernels_do_not_take():
    u8 = dict(dtype=torch.uint8)
    ok = torch.zeros((8, 8, 3), **u8)
    bad = {
        "dtype": [torch.zeros((8, 8, 3), dtype=torch.float32)],
        "channels": [torch.zeros((8, 8, 4), **u8)],
        "dims": [torch.zeros((8, 8), **u8)],
        "channel stride": [torch.zeros((8, 8, 6), **u8)[:, :, ::2]],
        "pixel stride": [torch.zeros((8, 16, 3), **u8)[:, ::2]],
        "planar": [torch.zeros((3, 8, 8), **u8).permute(1, 2, 0)],  # channel stride 64
        "overlapping rows": [torch.zeros((1, 8, 3), **u8).expand(8, 8, 3)],  # row stride 0
        "transposed": [torch.zeros((8, 8, 3), **u8).transpose(0, 1)],
        "empty": [torch.zeros((0, 8, 3), **u8)],
        "too many tiles": [torch.zeros((1, 1, 1), **u8).expand(64 * 64 + 1, 64 * 65, 3)],
        "one tensor of three dims": torch.zeros((8, 8, 3), **u8),
    }
    for name, frames in bad.items():
        with pytest.raises(ValueError):
            frame_table(frames)
        if isinstance(frames, list):
            with pytest.raises(ValueError):
                frame_table([ok] + frames)
    # rows laid out backwards: a negative stride cannot be built from a torch view, so the rule is fed what such a view would report
    class Backwards(torch.Tensor):
        def stride(self, dim=None):
            s = (-24, 3, 1)
            return s if dim is None else s[dim]

    with pytest.raises(ValueError, match="backwards or overlap"):
        frame_table([torch.zeros((8, 8, 3), **u8).as_subclass(Backwards)])
    with pytest.raises(ValueError, match="at most"):
        frame_table([ok] * (_lib.FRAME_MAX_COUNT + 1))


def test_frames_on_different_devices_are_refused():
    """Without a second device the rule is fed a meta tensor: another device, and metadata is all `frame_table` reads."""
    with pytest.raises(ValueError, match="frames\\[0\\] on"):
        frame_table([torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.uint8, device="meta")])


def _square(x0, y0, size, z):
    """Two triangles covering a square, three vertices each (six in all)."""
    x1, y1 = x0 + size, y0 + size
    return np.array([[x0, y0, z], [x1, y0, z], [x0, y1, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)


def test_the_head_drawn_second_wins_where_it_covers_also_from_behind(sim3dr_oracle):
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    near, far = _square(10.5, 10.5, 60, 50.0), _square(40.5, 30.5, 60, -50.0)  # `far` lies behind `near` and overlaps it
    col = [np.tile(np.float32([1.0, 0.0, 0.0]), (6, 1)), np.tile(np.float32([0.0, 0.0, 1.0]), (6, 1))]
    bg = np.full((120, 130, 3), 7, np.uint8)
    got = expected_frames(sim3dr_oracle, [bg], [near, far], tri, col, [0, 0])[0]
    solo_far = expected_frames(sim3dr_oracle, [bg], [far], tri, col[1:], [0])[0]
    solo_near = expected_frames(sim3dr_oracle, [bg], [near], tri, col[:1], [0])[0]
    cover_far, cover_near = (solo_far != bg).any(2), (solo_near != bg).any(2)
    assert (cover_far & cover_near).sum() > 500
    assert np.array_equal(got[cover_far], solo_far[cover_far])  # the second head's pixels, although it is the farther one
    assert np.array_equal(got[cover_near & ~cover_far], solo_near[cover_near & ~cover_far])
    assert np.array_equal(got[~cover_near & ~cover_far], bg[~cover_near & ~cover_far])
    # one shared z-buffer would have kept the nearer head: the reference does not
    shared, depth = sim3dr_oracle.rasterize(near, tri, col[0], bg=bg.copy(), return_depth=True)
    sim3dr_oracle.rasterize(far, tri, col[1], bg=shared, depth=depth)
    assert not np.array_equal(shared, got)
    # and the other order gives the other picture
    swapped = expected_frames(sim3dr_oracle, [bg], [far, near], tri, col[::-1], [0, 0])[0]
    assert np.array_equal(swapped[cover_near], solo_near[cover_near]) and not np.array_equal(swapped, got)
