"""Bounding boxes on the host: the argument forms of `FaceMeshPredictor.predict_boxes` and the rule `dad3d_preprocess_boxes` applies
to every box on the device (csrc/preprocess_boxes.hip), restated with `dataset.extend_bbox` / `ensure_bbox_boundaries` and
`resize_geometry`, so that a box the kernel would flag is refused before anything is launched; and `next_boxes`, the rule by which
`dad3d_boxes_from_heads` (csrc/track_boxes.hip) takes the boxes of the next call from the heads of this one; and `suppress_duplicates`,
the rule by which `dad3d_track_suppress_duplicates` (csrc/track_steady.hip) drops the later of two slots on one head; and
`assign_detections`, the rule by which `dad3d_track_assign_detections` (csrc/track_assign.hip) matches a detector's boxes to the slots,
spawns and retires. Pure numpy: no GPU, no library."""
from __future__ import annotations

from collections import namedtuple
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


AssignedDetections = namedtuple("AssignedDetections", "boxes flags image_index misses assign det_flags spawned")
MISSES_MAX = 2 ** 30


def assign_detections(boxes, flags, image_index, misses, det_boxes, det_index, n_frames: int, match_iou: float, count: Optional[int] = None,
                      frame_searched=None, refresh: bool = False, max_misses: Optional[int] = None) -> AssignedDetections:
    """Detections into tracks: `dad3d_track_assign_detections` (csrc/track_assign.hip, include/dad3d.h) on the host, rule for rule,
    in Python's integers. Slot state `boxes` int32 `[N,4]` as (x, y, w, h), `flags [N]`, `image_index [N]`, `misses [N]` (or None:
    nothing is counted and nothing retires); detections `det_boxes [M,4]`, `det_index [M]`, of which the first `count` are real
    (None: all; clamped to 0 .. M); `frame_searched [n_frames]` (None: every frame). -> copies of the slot state after the call,
    `assign [M]` (the slot of a matched or spawned detection, else -1), `det_flags [M]` (`_lib.ASSIGN_FLAG_*`, 0 for a match) and
    `spawned [N]` (1 where a slot was given to a new head).

    A slot is live if its flags are 0 and both sides positive, as it stands at entry; every other slot is free. A valid detection and
    a live slot of the same frame pass if `inter > 0` and `float(inter) >= match_iou * float(union)`, the comparison of
    `suppress_duplicates`. The passing pairs are sorted by the exact ratio inter / union, best first, ties by the lower detection,
    then the lower slot, and a pair is taken if neither side is taken: best-first, because "the first slot that passes" swaps two
    neighbouring heads whose boxes overlap. A taken slot has its misses cleared (and with `refresh` takes the detection's box). An
    unmatched detection that passes with any live slot is COVERED (its head has a track); the others take the slots that were free
    at entry, in order (SPAWNED), or are FULL. Two unmatched detections that overlap each other both spawn: that is the detector's
    own NMS to prevent, and `suppress_duplicates` takes what is left. A live slot that was searched for and not matched counts a
    miss (saturating at 2^30), and with more than `max_misses` (None: never) it is retired: `_lib.TRACK_FLAG_RETIRED`, the zero
    box, free from the next call on. Any number of slots and detections: the caps are the kernel's (its LDS), not the rule's."""
    out_boxes = np.array(boxes, dtype=np.int32).reshape(-1, 4)
    out_flags = np.array(flags, dtype=np.int32).reshape(-1)
    out_index = np.array(image_index, dtype=np.int32).reshape(-1)
    out_misses = None if misses is None else np.array(misses, dtype=np.int32).reshape(-1)
    dets = np.asarray(det_boxes, dtype=np.int32).reshape(-1, 4)
    det_frames = np.asarray(det_index, dtype=np.int32).reshape(-1)
    n, m = len(out_boxes), len(dets)
    if len(out_flags) != n or len(out_index) != n or (out_misses is not None and len(out_misses) != n):
        raise ValueError(f"flags / image_index / misses: expected {n} entries")
    if len(det_frames) != m:
        raise ValueError(f"det_index: expected {m} entries")
    iou, n_frames = float(match_iou), int(n_frames)
    if not 0.0 < iou <= 1.0:  # false for a NaN
        raise ValueError(f"match_iou {match_iou} is outside (0, 1]")
    if n_frames < 1:
        raise ValueError(f"n_frames {n_frames} is below 1")
    limit = -1 if max_misses is None else int(max_misses)
    if limit >= 0 and out_misses is None:
        raise ValueError(f"max_misses {max_misses} needs the misses it counts")
    searched = None if frame_searched is None else np.asarray(frame_searched).reshape(-1)
    if searched is not None and len(searched) != n_frames:
        raise ValueError(f"frame_searched: expected {n_frames} entries")
    real = m if count is None else min(max(int(count), 0), m)
    assign, det_flags, spawned = np.full(m, -1, np.int32), np.zeros(m, np.int32), np.zeros(n, np.int32)

    # int64 holds every value below: a corner is below 2^32 in magnitude, a side of the intersection below 2^31, an area below 2^62
    s64, d64 = out_boxes.astype(np.int64), dets.astype(np.int64)
    live = (out_flags == 0) & (s64[:, 2] > 0) & (s64[:, 3] > 0)
    valid = (np.arange(m) < real) & (d64[:, 2] > 0) & (d64[:, 3] > 0) & (det_frames >= 0) & (det_frames < n_frames)
    det_flags[~valid] = _lib.ASSIGN_FLAG_INVALID
    det_flags[real:] = _lib.ASSIGN_FLAG_PADDING
    iw = np.minimum((d64[:, 0] + d64[:, 2])[:, None], (s64[:, 0] + s64[:, 2])[None]) - np.maximum(d64[:, 0][:, None], s64[:, 0][None])
    ih = np.minimum((d64[:, 1] + d64[:, 3])[:, None], (s64[:, 1] + s64[:, 3])[None]) - np.maximum(d64[:, 1][:, None], s64[:, 1][None])
    both = valid[:, None] & live[None] & (det_frames[:, None] == out_index[None]) & (iw > 0) & (ih > 0)
    inter = np.where(both, iw, 0) * np.where(both, ih, 0)
    union = np.where(both, (d64[:, 2] * d64[:, 3])[:, None] + (s64[:, 2] * s64[:, 3])[None] - inter, 1)
    passing = both & (inter.astype(np.float64) >= iou * union.astype(np.float64))  # int64 -> float64 rounds to nearest even, as the device's
    covered = passing.any(axis=1)
    pair_d, pair_s = np.nonzero(passing)  # ascending in (d, s)
    # the exact ratio as one integer: two different ratios of numbers below 2^63 lie more than 2^-126 apart, so their floors at
    # 128 fractional bits differ and keep their order, and equal ratios give equal floors. The sort is stable: ties stay in (d, s) order.
    ratio = [(int(i) << 128) // int(u) for i, u in zip(inter[pair_d, pair_s], union[pair_d, pair_s])]
    matched = np.zeros(n, bool)
    for k in sorted(range(len(ratio)), key=lambda k: -ratio[k]):
        d, s = int(pair_d[k]), int(pair_s[k])
        if assign[d] < 0 and not matched[s]:
            assign[d], matched[s] = s, True
            if out_misses is not None:
                out_misses[s] = 0
            if refresh:
                out_boxes[s] = dets[d]
    vacant = [s for s in range(n) if not live[s]]  # free at entry, ascending
    rank = 0
    for d in range(m):
        if not valid[d] or assign[d] >= 0:
            continue
        if covered[d]:
            det_flags[d] = _lib.ASSIGN_FLAG_COVERED
        elif rank < len(vacant):
            s = vacant[rank]
            rank += 1
            out_boxes[s], out_index[s], out_flags[s], spawned[s] = dets[d], det_frames[d], 0, 1
            if out_misses is not None:
                out_misses[s] = 0
            assign[d], det_flags[d] = s, _lib.ASSIGN_FLAG_SPAWNED
        else:
            det_flags[d] = _lib.ASSIGN_FLAG_FULL
    if out_misses is not None:
        for s in range(n):
            if not live[s] or matched[s]:
                continue
            frame = int(out_index[s])
            if searched is not None and not (0 <= frame < n_frames and searched[frame] != 0):
                continue
            seen = int(out_misses[s])
            now = MISSES_MAX if seen >= MISSES_MAX else seen + 1
            out_misses[s] = now
            if limit >= 0 and now > limit:
                out_flags[s] = _lib.TRACK_FLAG_RETIRED
                out_boxes[s] = 0
    return AssignedDetections(out_boxes, out_flags, out_index, out_misses, assign, det_flags, spawned)


def check_boxes(shapes: Sequence[Tuple[int, int]], flat: np.ndarray, index: np.ndarray, factors, img_size: int) -> None:
    """ValueError naming the first host box the kernel would flag. Nothing here touches the device."""
    for k, (box, image) in enumerate(zip(flat, index)):
        crop, flags = crop_and_flags(box, int(image), shapes, factors, img_size)
        if flags:
            where = f"of frame {int(image)} ({shapes[image][0]} x {shapes[image][1]})" if 0 <= image < len(shapes) else f"with image_index {int(image)}"
            raise ValueError(f"box {k} {box.tolist()} {where}: {FLAG_NAMES[flags]}"
                             + (f" (crop {crop.tolist()})" if flags != _lib.BOX_FLAG_RANGE else ""))
