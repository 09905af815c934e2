"""CPU: the host side of `FaceMeshPredictor.predict_boxes` (dad_3dheads_amd/boxes.py) -- the argument forms, and the rule that refuses a box
the kernel would flag before anything is launched. The table of boxes, frames and hand-derived flags is the GPU test's
(tests/test_gpu_predict_boxes.py), so the host check and the kernel are held to the same cases."""
import numpy as np
import pytest
import torch

import test_gpu_predict_boxes as table
from dad_3dheads_amd import _lib, boxes, resize_geometry
from dad_3dheads_amd.dataset import extend_bbox


def test_the_examples_of_the_rule():
    assert extend_bbox(np.array([3.0, -2.0, 15.0, 17.0]), 0.1).tolist() == [1, -3, 18, 20]  # -3.7 goes to -3, not to -4
    assert resize_geometry.py3round(5 * (256 / 512.0)) == 2 and resize_geometry.py3round(7 * (256 / 512.0)) == 4
    assert resize_geometry.py3round(1 * (256 / 1000.0)) == 0


def test_rint_is_py3round():
    """The kernel rounds `dim * scale` with rint (half to even); albumentations' py3round is the same function on 0 .. 4000 in quarter steps."""
    x = np.arange(0, 4000 * 4 + 1) / 4.0
    assert np.rint(x).astype(np.int64).tolist() == [resize_geometry.py3round(float(v)) for v in x]


@pytest.mark.parametrize("dtype", list(table.NP_DTYPES))
def test_host_rule_gives_the_crops_and_flags_of_the_table(dtype):
    for offset in table.CASES:
        b, index, want_flags = table._cases(offset, table.NP_DTYPES[dtype])
        want_crops, _ = table._expected(b, index, want_flags, offset, 256)
        for k in range(len(b)):
            crop, flags = boxes.crop_and_flags(b[k], int(index[k]), table.SHAPES, boxes.offset_factors(offset), 256)
            assert flags == want_flags[k] and crop.dtype == np.int32 and np.array_equal(crop, want_crops[k]), (offset, k)


def test_offset_forms():
    assert boxes.offset_factors(None) is None
    assert boxes.offset_factors(0.1) == (0.1, 0.1, 0.1, 0.1)
    assert boxes.offset_factors((0.1, 0.2)) == (0.1, 0.1, 0.2, 0.2)  # (w, h) -> left = right, top = bottom
    assert boxes.offset_factors((0.05, 0.2, 0.1, 0.3)) == (0.05, 0.2, 0.1, 0.3)
    assert boxes.offset_factors([1, 2]) == (1.0, 1.0, 2.0, 2.0)
    for bad in ((0.1, 0.2, 0.3), float("nan"), (0.1, float("inf"))):
        with pytest.raises(ValueError, match="offset"):
            boxes.offset_factors(bad)
    # every form is extend_bbox's own reading of it
    box = np.array([30.0, 40.0, 50.0, 60.0])
    for form in (0.1, (0.1, 0.2), (0.05, 0.2, 0.1, 0.3)):
        assert extend_bbox(box, form).tolist() == extend_bbox(box, boxes.offset_factors(form)).tolist()


def test_list_per_frame_and_flat_with_index_are_one_form():
    per_frame = [np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.int32), np.zeros((0, 4)), np.array([[9, 10, 11, 12]], np.int32)]
    flat, index = boxes.flatten_boxes(3, per_frame)
    assert flat.dtype == np.int32 and flat.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]] and index.tolist() == [0, 0, 2]
    flat2, index2 = boxes.flatten_boxes(3, flat, image_index=[0, 0, 2])
    assert flat2.dtype == flat.dtype and np.array_equal(flat2, flat) and index2.dtype == np.int32 and index2.tolist() == [0, 0, 2]
    mixed, _ = boxes.flatten_boxes(2, [np.array([[1, 2, 3, 4]], np.int32), np.array([[1.5, 2, 3, 4]])])
    assert mixed.dtype == np.float64
    for dtype in (np.int32, np.int64, np.float32, np.float64):
        assert boxes.flatten_boxes(1, [np.ones((2, 4), dtype)])[0].dtype == dtype  # uploaded as they are
    assert boxes.flatten_boxes(1, [np.ones((2, 4), np.uint8)])[0].dtype == np.float64
    assert boxes.flatten_boxes(1, [[[1, 2, 3, 4]]])[0].tolist() == [[1, 2, 3, 4]]
    assert boxes.flatten_boxes(2, [[], []])[0].shape == (0, 4)
    assert boxes.flatten_boxes(2, np.ones((3, 4)), image_index=np.array([0, 5, -7]))[1].tolist() == [0, 5, -1]
    for bad in (lambda: boxes.flatten_boxes(2, [np.ones((1, 4))]), lambda: boxes.flatten_boxes(1, np.ones((2, 4)), image_index=[0]),
                lambda: boxes.flatten_boxes(1, np.ones((2, 3)), image_index=[0, 0]), lambda: boxes.flatten_boxes(1, np.ones((1, 4)), image_index=[0.5])):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("box, image, word", [((200, 200, 10, 10), 0, "empty"), ((5, 100, 1000, 1), 1, "0 pixels"),
                                              ((float("nan"), 0, 10, 10), 0, "not finite"), ((0, 0, 2 ** 30, 5), 0, "2\\^30"),
                                              ((5, 5, 10, 10), 2, "image_index 2")])
def test_a_flagged_host_box_is_a_value_error_that_names_it(box, image, word):
    shapes = [(97, 131), (520, 1010)]
    good = [10.0, 10.0, 20.0, 20.0]
    flat, index = np.array([good, box, good], np.float64), np.array([0, image, 1], np.int32)
    with pytest.raises(ValueError, match=f"box 1 .*{word}"):
        boxes.check_boxes(shapes, flat, index, None, 256)
    boxes.check_boxes(shapes, flat[[0, 2]], index[[0, 2]], boxes.offset_factors(0.1), 256)  # the good ones pass
    assert boxes.crop_and_flags(good, 1, shapes, boxes.offset_factors(0.1), 256)[0].tolist() == [8, 8, 24, 24]


def test_predict_boxes_refuses_before_it_touches_the_device():
    """The check stands in front of every upload and launch: an object without a device or a library gets as far as the ValueError."""
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    pred = object.__new__(FaceMeshPredictor)
    pred._img_size = 256
    frames = [torch.zeros((97, 131, 3), dtype=torch.uint8), torch.zeros((64, 64, 3), dtype=torch.uint8)]
    with pytest.raises(ValueError, match="box 2 .*frame 1"):
        pred._predict_boxes_staged(frames, [np.array([[5, 5, 20, 20], [50, 5, 20, 20]]), np.array([[70, 5, 20, 20]])], None, None, False, False)
    with pytest.raises(ValueError, match="offset"):
        pred._predict_boxes_staged(frames, [np.zeros((0, 4)), np.zeros((0, 4))], None, (1, 2, 3), False, False)
    assert _lib.BOX_FLAG_EMPTY | _lib.BOX_FLAG_COLLAPSED | _lib.BOX_FLAG_RANGE == 7
