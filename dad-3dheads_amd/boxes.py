"""Bounding boxes on the host: the argument forms of `FaceMeshPredictor.predict_boxes` and the rule `dad3d_preprocess_boxes` applies
to every box on the device (csrc/preprocess_boxes.hip), restated with `dataset.extend_bbox` / `ensure_bbox_boundaries` and
`resize_geometry`, so that a box the kernel would flag is refused before anything is launched; and `next_boxes`, the rule by which
`dad3d_boxes_from_heads` (csrc/track_boxes.hip) takes the boxes of the next call from the heads of this one; and `suppress_duplicates`,
the rule by which `dad3d_track_suppress_duplicates` (csrc/track_steady.hip) drops the later of two slots on one head. Pure numpy: no GPU,
no library."""
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


def next_boxes(proj, shapes: Sequence[Tuple[int, int]], image_index, prev_flags=None, subset=None, min_side: int = 1,
               min_visible: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """The boxes of the next call from the projected vertices of this one: `dad3d_boxes_from_heads` (csrc/track_boxes.hip,
    include/dad3d.h) on the host, rule for rule. `proj` float32 `[N,V,>=2]` (x, y first), `shapes` the frames' (h, w), `image_index
    [N]`, `prev_flags [N]` the flags of the call that produced `proj` (or None), `subset` vertex indices to bound (None: all; duplicates
    allowed) -> (int32 `[N,4]` boxes as (x, y, w, h), int32 `[N]` of `_lib.TRACK_FLAG_*`). Any flag zeroes the box, which the next
    `crop_and_flags` flags EMPTY: a lost head stays lost in its slot until the caller writes a fresh box there.

    `min_side=1` asks for no more than "not empty" and `min_visible=0.5` for most of the head's box still in the frame; both are
    design choices, not measurements, and the caller's to set."""
    proj = np.asarray(proj)
    if proj.ndim != 3 or proj.shape[2] < 2 or proj.shape[1] < 1 or proj.dtype != np.float32:
        raise ValueError(f"proj: expected float32 [N,V,2] or [N,V,3], got {proj.dtype} {proj.shape}")
    n, n_verts = proj.shape[:2]
    index = np.asarray(image_index).reshape(-1)
    previous = None if prev_flags is None else np.asarray(prev_flags).reshape(-1)
    if len(index) != n or (previous is not None and len(previous) != n):
        raise ValueError(f"image_index / prev_flags: expected {n} entries")
    if int(min_side) < 0 or not 0.0 <= float(min_visible) <= 1.0:  # false for a NaN
        raise ValueError(f"min_side {min_side} is negative or min_visible {min_visible} is outside [0, 1]")
    picked = None if subset is None else np.asarray(subset).reshape(-1).astype(np.int64)
    if picked is not None and len(picked) == 0:
        raise ValueError("subset: no index (None selects all vertices)")
    boxes, flags = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    for i in range(n):
        if previous is not None and previous[i] != 0:
            flags[i] = _lib.TRACK_FLAG_PREVIOUS
            continue
        image = int(index[i])
        if not 0 <= image < len(shapes) or not all(0 < int(s) < 2 ** 30 for s in shapes[image][:2]) \
                or (picked is not None and not np.all((picked >= 0) & (picked < n_verts))):
            flags[i] = _lib.TRACK_FLAG_RANGE
            continue
        xy = proj[i, :, :2] if picked is None else proj[i, picked, :2]
        if not np.all(np.isfinite(xy)):
            flags[i] = _lib.TRACK_FLAG_NONFINITE
            continue
        lo, hi = xy.min(axis=0), xy.max(axis=0)  # float32, exact
        if not (np.all(np.abs(lo) < RANGE) and np.all(np.abs(hi) < RANGE)):
            flags[i] = _lib.TRACK_FLAG_RANGE
            continue
        x0, y0 = (int(v) for v in np.floor(lo))
        x1, y1 = (int(v) for v in np.ceil(hi))
        w, h = x1 - x0, y1 - y0
        frame_h, frame_w = (int(s) for s in shapes[image][:2])
        if min(w, h) < int(min_side):
            flags[i] |= _lib.TRACK_FLAG_SMALL
        if w * h != 0:
            inter = max(0, min(x1, frame_w) - max(x0, 0)) * max(0, min(y1, frame_h) - max(y0, 0))
            if float(inter) < float(min_visible) * float(w * h):  # Python's float(int) rounds to nearest even, as the conversion on the device
                flags[i] |= _lib.TRACK_FLAG_OUTSIDE
        if not flags[i]:
            boxes[i] = (x0, y0, w, h)
    return boxes, flags


def suppress_duplicates(boxes, flags, image_index, merge_iou: float) -> Tuple[np.ndarray, np.ndarray]:
    """Two slots on one head: `dad3d_track_suppress_duplicates` (csrc/track_steady.hip, include/dad3d.h) on the host, rule for rule.
    `boxes` int32 `[N,4]` as (x, y, w, h) and `flags [N]` as `next_boxes` left them, `image_index [N]` -> copies of both with every
    duplicate flagged `_lib.TRACK_FLAG_DUPLICATE` and zeroed. A slot takes part only if its flags are 0 and both sides are positive.
    Walking upward, slot j is a duplicate if a KEPT earlier slot of the same frame overlaps it with `inter > 0` and
    `float(inter) >= merge_iou * float(union)`, areas as integers: greedy, so a slot that was suppressed suppresses nobody, and the
    lower slot wins -- an arbitrary but fixed choice, since which of two converged slots is the right one cannot be known without
    appearance. Any number of slots: `_lib.TRACK_MAX_SLOTS` is the kernel's limit (its LDS), not the rule's."""
    out_boxes = np.array(boxes, dtype=np.int32).reshape(-1, 4)
    out_flags = np.array(flags, dtype=np.int32).reshape(-1)
    index = np.asarray(image_index).reshape(-1)
    n = len(out_boxes)
    if len(out_flags) != n or len(index) != n:
        raise ValueError(f"flags / image_index: expected {n} entries")
    iou = float(merge_iou)
    if not 0.0 < iou <= 1.0:  # false for a NaN
        raise ValueError(f"merge_iou {merge_iou} is outside (0, 1]")
    kept = []  # (frame, x0, y0, x1, y1, area) in Python's integers
    for j in range(n):
        x, y, w, h = (int(v) for v in out_boxes[j])
        if out_flags[j] != 0 or w <= 0 or h <= 0:
            continue
        frame, x1, y1, area = int(index[j]), x + w, y + h, w * h
        for f, ax0, ay0, ax1, ay1, a_area in kept:
            if f != frame:
                continue
            inter = max(0, min(ax1, x1) - max(ax0, x)) * max(0, min(ay1, y1) - max(ay0, y))
            if inter > 0 and float(inter) >= iou * float(a_area + area - inter):  # float(int) rounds to nearest even, as the device's conversion
                out_boxes[j] = 0
                out_flags[j] = _lib.TRACK_FLAG_DUPLICATE
                break
        else:
            kept.append((frame, x, y, x1, y1, area))
    return out_boxes, out_flags


def check_boxes(shapes: Sequence[Tuple[int, int]], flat: np.ndarray, index: np.ndarray, factors, img_size: int) -> None:
    """ValueError naming the first host box the kernel would flag. Nothing here touches the device."""
    for k, (box, image) in enumerate(zip(flat, index)):
        crop, flags = crop_and_flags(box, int(image), shapes, factors, img_size)
        if flags:
            where = f"of frame {int(image)} ({shapes[image][0]} x {shapes[image][1]})" if 0 <= image < len(shapes) else f"with image_index {int(image)}"
            raise ValueError(f"box {k} {box.tolist()} {where}: {FLAG_NAMES[flags]}"
                             + (f" (crop {crop.tolist()})" if flags != _lib.BOX_FLAG_RANGE else ""))
