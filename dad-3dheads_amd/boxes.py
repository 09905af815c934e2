"""Bounding boxes on the host: the argument forms of `FaceMeshPredictor.predict_boxes` and the rule `dad3d_preprocess_boxes` applies
to every box on the device (csrc/preprocess_boxes.hip), restated with `dataset.extend_bbox` / `ensure_bbox_boundaries` and
`resize_geometry`, so that a box the kernel would flag is refused before anything is launched. Pure numpy: no GPU, no library."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .dataset import ensure_bbox_boundaries, extend_bbox
from .resize_geometry import longest_max_size

Offset = Union[None, float, Tuple[float, float], Tuple[float, float, float, float]]
BOX_DTYPES = {np.dtype(np.int32): _lib.BOX_DTYPE_I32, np.dtype(np.int64): _lib.BOX_DTYPE_I64,
              np.dtype(np.float32): _lib.BOX_DTYPE_F32, np.dtype(np.float64): _lib.BOX_DTYPE_F64}
RANGE = float(2 ** 30)
FLAG_NAMES = {_lib.BOX_FLAG_EMPTY: "the crop is empty after the boundary rule", _lib.BOX_FLAG_COLLAPSED: "the resized crop has a side of 0 pixels",
              _lib.BOX_FLAG_RANGE: "a value is not finite, is 2^30 or beyond, or the image index is outside the frames"}


def offset_factors(offset: Offset) -> Optional[Tuple[float, float, float, float]]:
    """`extend_bbox`'s offset forms (data/utils.py:73-103) as (left, right, top, bottom): one value, (w, h), or the four; None stays None."""
    if offset is None:
        return None
    if isinstance(offset, (tuple, list)):
        if len(offset) == 4:
            left, right, top, bottom = offset
        elif len(offset) == 2:
            left = right = offset[0]
            top = bottom = offset[1]
        else:
            raise ValueError(f"offset: expected one value, 2 or 4 of them, got {len(offset)}")
    else:
        left = right = top = bottom = offset
    factors = tuple(float(v) for v in (left, right, top, bottom))
    if not all(np.isfinite(factors)):
        raise ValueError(f"offset: {offset!r} is not finite")
    return factors


def flatten_boxes(n_frames: int, boxes, image_index=None) -> Tuple[np.ndarray, np.ndarray]:
    """Host boxes in either form -> ([N,4] of int32, int64, float32 or float64, int32 [N]): a list with one `[k_i,4]` array per frame
    (`image_index` None), or one `[N,4]` array with `image_index [N]`. Any other dtype becomes float64."""
    if image_index is None:
        if len(boxes) != n_frames:
            raise ValueError(f"boxes: without image_index expected one [k,4] array per frame ({n_frames}), got {len(boxes)} items")
        per_frame = [np.asarray(b).reshape(-1, 4) if np.size(b) else np.zeros((0, 4), np.int32) for b in boxes]
        index = np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(per_frame)]) if per_frame else np.zeros(0, np.int32)
        filled = [b for b in per_frame if len(b)]
        flat = np.concatenate(filled) if filled else np.zeros((0, 4), np.int32)  # mixed dtypes: numpy's common type
    else:
        flat = np.asarray(boxes)
        index = np.asarray(image_index)
        if flat.ndim != 2 or flat.shape[1] != 4 or index.shape != (flat.shape[0],):
            raise ValueError(f"boxes: expected [N,4] with image_index [N], got {flat.shape} and {index.shape}")
        if index.dtype.kind not in "iu":
            raise ValueError(f"image_index: expected integers, got {index.dtype}")
        index = index.astype(np.int64)
        index = np.where((index < 0) | (index > 2 ** 31 - 1), -1, index).astype(np.int32)  # outside the frames either way
    if flat.dtype not in BOX_DTYPES:
        if flat.dtype.kind not in "iuf":
            raise ValueError(f"boxes: expected numbers, got {flat.dtype}")
        flat = flat.astype(np.float64)
    return np.ascontiguousarray(flat), np.ascontiguousarray(index)


def crop_and_flags(box, image: int, shapes: Sequence[Tuple[int, int]], factors: Optional[Tuple[float, float, float, float]],
                   img_size: int) -> Tuple[np.ndarray, int]:
    """The crop (x, y, w, h) int32 and the DAD3D_BOX_FLAG_* of one box, as the kernel computes them."""
    zero = np.zeros(4, np.int32)
    v = np.asarray(box).astype(np.float64)
    if not (0 <= image < len(shapes)) or not np.all(np.abs(v) < RANGE):  # a NaN compares false
        return zero, _lib.BOX_FLAG_RANGE
    if factors is not None:
        x, y, w, h = v
        left, right, top, bottom = factors
        with np.errstate(all="ignore"):
            grown = np.array([x - w * left, y - h * top, w * (1.0 + right + left), h * (1.0 + top + bottom)])
        if not np.all(np.abs(grown) < RANGE):
            return zero, _lib.BOX_FLAG_RANGE
        v = extend_bbox(v, factors)
    crop = ensure_bbox_boundaries(v.astype(np.int32), shapes[image])
    if crop[2] <= 0 or crop[3] <= 0:
        return crop, _lib.BOX_FLAG_EMPTY
    new_h, new_w, _, _ = longest_max_size(int(crop[3]), int(crop[2]), img_size)
    return crop, (_lib.BOX_FLAG_COLLAPSED if new_h == 0 or new_w == 0 else 0)


def check_boxes(shapes: Sequence[Tuple[int, int]], flat: np.ndarray, index: np.ndarray, factors, img_size: int) -> None:
    """ValueError naming the first host box the kernel would flag. Nothing here touches the device."""
    for k, (box, image) in enumerate(zip(flat, index)):
        crop, flags = crop_and_flags(box, int(image), shapes, factors, img_size)
        if flags:
            where = f"of frame {int(image)} ({shapes[image][0]} x {shapes[image][1]})" if 0 <= image < len(shapes) else f"with image_index {int(image)}"
            raise ValueError(f"box {k} {box.tolist()} {where}: {FLAG_NAMES[flags]}"
                             + (f" (crop {crop.tolist()})" if flags != _lib.BOX_FLAG_RANGE else ""))
