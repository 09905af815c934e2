"""CPU: tracking heads from frame to frame -- `dad3d_boxes_from_heads` is exported and its flags are the header's, the host statement
of its rule (`boxes.next_boxes`) is pinned by hand, every flagged head's zero box is one that `crop_and_flags` flags EMPTY, and
`HeadTracker` refuses bad calls before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dad_3dheads_amd import _lib, boxes
from dad_3dheads_amd.tracking import HeadTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R, NF, S, O = (_lib.TRACK_FLAG_PREVIOUS, _lib.TRACK_FLAG_RANGE, _lib.TRACK_FLAG_NONFINITE, _lib.TRACK_FLAG_SMALL,
                  _lib.TRACK_FLAG_OUTSIDE)
FRAME = [(100, 200)]  # (h, w)


def _one(points, shapes=FRAME, image=0, **kw):
    """next_boxes on one head given by its (x, y) list -> (box as a list, flags)."""
    proj = np.asarray(points, np.float32).reshape(1, -1, 2)
    b, f = boxes.next_boxes(proj, shapes, [image], **kw)
    assert b.dtype == np.int32 and f.dtype == np.int32 and b.shape == (1, 4) and f.shape == (1,)
    return b[0].tolist(), int(f[0])


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_and_flags_mirror_the_header():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dad3d_boxes_from_heads")
    assert "dad3d_boxes_from_heads" in _lib.SIGNATURES and len(_lib.SIGNATURES["dad3d_boxes_from_heads"][1]) == 17
    text = open(os.path.join(ROOT, "include", "dad3d.h")).read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+DAD3D_(TRACK_FLAG_[A-Z]+)\s+(0x[0-9a-fA-F]+|\d+)\b", text)}
    assert sorted(defines) == ["TRACK_FLAG_NONFINITE", "TRACK_FLAG_OUTSIDE", "TRACK_FLAG_PREVIOUS", "TRACK_FLAG_RANGE", "TRACK_FLAG_SMALL"]
    for name, value in defines.items():
        assert getattr(_lib, name) == value, name
    assert len(set(defines.values())) == 5 and all(v and v & (v - 1) == 0 for v in defines.values())  # five different bits


def test_argument_errors_come_before_any_device_work():
    """No GPU is needed to be refused."""
    lib = _lib.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)

    def call(proj=p, n=1, v=1, hs=2, vs=2, subset=None, ns=0, frames=p, m=1, index=p, prev=None, side=1, vis=0.5, out=p, flags=p):
        return lib.dad3d_boxes_from_heads(proj, n, v, hs, vs, subset, ns, frames, m, index, prev, side, vis, out, flags, 0, None)

    assert call(n=0) == _lib.OK
    for kw in ({"proj": None}, {"frames": None}, {"index": None}, {"out": None}, {"flags": None}, {"n": -1}, {"n": 65536}, {"v": 0},
               {"v": 65536}, {"m": 0}, {"m": 65536}, {"subset": p, "ns": 65536}, {"subset": p, "ns": 0}, {"ns": 3}, {"vs": 1}, {"side": -1},
               {"vis": -0.01}, {"vis": 1.01}, {"vis": float("nan")}):
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"dad3d_boxes_from_heads" in lib.dad3d_last_error()


# ---- the rule, by hand ---------------------------------------------------------------------------------------------------------
def test_one_vertex_is_an_empty_box_and_small():
    assert _one([(3.0, 4.0)], min_side=0) == ([3, 4, 0, 0], 0)  # the box itself; w * h == 0, so OUTSIDE is not evaluated
    assert _one([(3.0, 4.0)], min_side=1) == ([0, 0, 0, 0], S)


def test_floor_and_ceil_of_two_vertices():
    assert _one([(-0.5, 2.25), (7.0, 9.0)]) == ([-1, 2, 8, 7], 0)  # floor(-0.5) = -1, ceil(7.0) = 7; 7 of 8 columns are in the frame
    assert _one([(7.0, 9.0), (-0.5, 2.25)]) == ([-1, 2, 8, 7], 0)
    assert _one([(-0.0, 0.0), (3.0, 3.0)]) == ([0, 0, 3, 3], 0)


def test_nan_in_the_last_of_5023_vertices():
    pts = np.tile(np.array([[10.0, 20.0], [30.0, 50.0]], np.float32), (2512, 1))[:5023]
    assert _one(pts) == ([10, 20, 20, 30], 0)
    for bad in (np.nan, np.inf, -np.inf):
        for axis in (0, 1):
            q = pts.copy()
            q[-1, axis] = bad
            assert _one(q) == ([0, 0, 0, 0], NF), (bad, axis)


def test_range_at_two_to_the_thirty():
    below = float(np.nextafter(np.float32(2 ** 30), np.float32(0)))
    assert below == 2 ** 30 - 64
    assert _one([(0.0, 0.0), (2.0 ** 30, 10.0)]) == ([0, 0, 0, 0], R)
    assert _one([(0.0, -(2.0 ** 30)), (10.0, 10.0)]) == ([0, 0, 0, 0], R)
    box, flags = _one([(0.0, 0.0), (below, 10.0)], min_visible=0.0)
    assert flags == 0 and box == [0, 0, 2 ** 30 - 64, 10]
    assert _one([(0.0, 0.0), (below, 10.0)])[1] == O  # in range, and almost wholly outside a frame 200 wide


def test_index_frame_and_subset_errors_are_range():
    pts = [(10.0, 10.0), (20.0, 30.0)]
    assert _one(pts, image=-1) == ([0, 0, 0, 0], R)
    assert _one(pts, image=1) == ([0, 0, 0, 0], R)
    assert _one(pts, shapes=[(0, 200)]) == ([0, 0, 0, 0], R)
    assert _one(pts, shapes=[(100, 2 ** 30)]) == ([0, 0, 0, 0], R)
    assert _one(pts, subset=[0, 2]) == ([0, 0, 0, 0], R)
    assert _one(pts, subset=[-1]) == ([0, 0, 0, 0], R)
    assert _one(pts, subset=[1, 1, 0]) == ([10, 10, 10, 20], 0)
    assert _one([(10.0, 10.0), (np.nan, 30.0), (20.0, 30.0)], subset=[0, 2, 2]) == ([10, 10, 10, 20], 0)  # the NaN is not selected


def test_previous_comes_first_and_reads_nothing():
    proj = np.full((2, 4, 2), np.nan, np.float32)
    proj[1] = [[1, 1], [9, 9], [1, 9], [9, 1]]
    b, f = boxes.next_boxes(proj, FRAME, [5, 0], prev_flags=[_lib.BOX_FLAG_EMPTY, 0])
    assert f.tolist() == [P, 0] and b.tolist() == [[0, 0, 0, 0], [1, 1, 8, 8]]


def test_min_visible_boundary_on_a_box_half_in_the_frame():
    pts = [(-10.0, 10.0), (10.0, 30.0)]  # 20 x 20, columns 0 .. 9 in the frame: inter = 200 of 400
    assert _one(pts, min_visible=0.5) == ([-10, 10, 20, 20], 0)
    assert _one(pts, min_visible=float(np.nextafter(0.5, 1))) == ([0, 0, 0, 0], O)
    assert _one(pts, min_visible=1.0) == ([0, 0, 0, 0], O)
    assert _one([(0.0, 0.0), (200.0, 100.0)], min_visible=1.0) == ([0, 0, 200, 100], 0)  # the frame itself
    assert _one([(0.0, 0.0), (200.0, 100.5)], min_visible=1.0) == ([0, 0, 0, 0], O)


def test_small_and_outside_together():
    assert _one([(-30.0, 5.0), (-10.0, 7.0)], min_side=3) == ([0, 0, 0, 0], S | O)
    assert _one([(-30.0, 5.0), (-10.0, 7.0)], min_side=2) == ([0, 0, 0, 0], O)
    assert _one([(30.0, 5.0), (50.0, 7.0)], min_side=3) == ([0, 0, 0, 0], S)


def test_a_head_outside_the_frame_is_lost_where_the_boundary_rule_alone_locks_onto_the_corner():
    """`ensure_bbox_boundaries` moves the box (-50, -50, 20, 20) to the frame's corner and keeps a valid crop there: a head that has
    walked out of the frame would be tracked in the corner for ever. `next_boxes` flags it OUTSIDE instead."""
    crop, flags = boxes.crop_and_flags([-50, -50, 20, 20], 0, FRAME, boxes.offset_factors(0.1), 256)
    assert crop.tolist() == [0, 0, 24, 24] and flags == 0
    assert _one([(-50.0, -50.0), (-30.0, -30.0)], min_visible=0.0) == ([-50, -50, 20, 20], 0)  # the box the head gives
    assert _one([(-50.0, -50.0), (-30.0, -30.0)]) == ([0, 0, 0, 0], O)


@pytest.mark.parametrize("offset", [None, 0.1])
def test_every_flagged_head_gives_a_box_the_preprocess_rule_flags_empty(offset):
    heads = {P: ([(10.0, 10.0), (20.0, 20.0)], {"prev_flags": [1]}), R: ([(10.0, 10.0), (2.0 ** 30, 20.0)], {}),
             NF: ([(10.0, np.inf), (20.0, 20.0)], {}), S: ([(10.0, 10.0), (20.0, 10.0)], {}), O: ([(-50.0, 10.0), (-30.0, 20.0)], {}),
             S | O: ([(-50.0, 10.0), (-30.0, 10.5)], {"min_side": 2})}
    for want, (pts, kw) in heads.items():
        box, flags = _one(pts, **kw)
        assert flags == want and box == [0, 0, 0, 0], (want, flags, box)
        crop, crop_flags = boxes.crop_and_flags(box, 0, FRAME, boxes.offset_factors(offset), 256)
        assert crop_flags == _lib.BOX_FLAG_EMPTY and crop.tolist() == [0, 0, 0, 0], want


def test_next_boxes_refuses_bad_arguments():
    proj = np.zeros((2, 3, 2), np.float32)
    for args, kw in (((proj.astype(np.float64), FRAME, [0, 0]), {}), ((proj[:, :, :1], FRAME, [0, 0]), {}), ((proj, FRAME, [0]), {}),
                     ((proj, FRAME, [0, 0]), {"prev_flags": [0]}), ((proj, FRAME, [0, 0]), {"min_side": -1}),
                     ((proj, FRAME, [0, 0]), {"min_visible": float("nan")}), ((proj, FRAME, [0, 0]), {"subset": []})):
        with pytest.raises(ValueError):
            boxes.next_boxes(*args, **kw)
    three = np.zeros((1, 2, 3), np.float32)  # [N,V,3]: z is ignored
    three[0] = [[1, 2, 1e9], [5, 9, np.nan]]
    b, f = boxes.next_boxes(three, FRAME, [0])
    assert b.tolist() == [[1, 2, 4, 7]] and f.tolist() == [0]


# ---- HeadTracker's argument errors ---------------------------------------------------------------------------------------------
class _NoLaunch:
    """A predictor on the CPU whose every launch is an error: what the tracker may touch before it refuses a call."""
    device = torch.device("cpu")
    _img_size = 256

    def __getattr__(self, name):
        raise AssertionError(f"the tracker reached for predictor.{name}")


def test_tracker_refuses_before_anything_is_launched():
    frames = [np.zeros((96, 128, 3), np.uint8), np.zeros((64, 64, 3), np.uint8)]
    tracker = HeadTracker(_NoLaunch())
    with pytest.raises(ValueError, match="start"):
        tracker.step(frames)
    with pytest.raises(ValueError, match="start"):
        tracker.reseed([0], [[1, 1, 5, 5]])
    with pytest.raises(ValueError, match="start"):
        tracker.lost()
    with pytest.raises(ValueError, match="box 1 "):  # a host box that predict_boxes would refuse
        tracker.start(frames, [np.array([[10, 10, 30, 30], [500, 10, 30, 30]]), np.zeros((0, 4))])
    tracker.start(frames, [np.array([[10, 10, 30, 30], [40, 20, 50, 60]]), np.array([[5, 5, 40, 40]])])
    assert tracker.n_slots == 3 and tracker.lost().tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="frames"):
        tracker.step(frames[:1])
    with pytest.raises(ValueError, match="frames"):
        tracker.step(frames + frames[:1])
    for slots in ([3], [-1], [0, 7], [0.5]):
        with pytest.raises(ValueError, match="slots"):
            tracker.reseed(slots, [[1, 1, 5, 5]] * len(slots))
    with pytest.raises(ValueError, match="boxes"):
        tracker.reseed([0, 1], [[1, 1, 5, 5]])
    assert tracker._boxes.tolist() == [[10, 10, 30, 30], [40, 20, 50, 60], [5, 5, 40, 40]]  # nothing moved
    tracker.reseed([2, 0], [[7, 8, 9, 10], [1, 2, 3, 4]])
    assert tracker._boxes.tolist() == [[1, 2, 3, 4], [40, 20, 50, 60], [7, 8, 9, 10]]
    for kw in ({"min_side": -1}, {"min_visible": 1.5}, {"subset": []}, {"subset": [0.5]}, {"offset": (1, 2, 3)}):
        with pytest.raises(ValueError):
            HeadTracker(_NoLaunch(), **kw)
