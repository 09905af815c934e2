"""LongestMaxSize + PadIfNeeded geometry (albumentations `py3round`, model_training/model/utils.py `calculate_paddings`), shared by
the predictor's preprocessing and the training-batch collate. Pure Python: safe to import in a forked DataLoader worker."""
from __future__ import annotations

from typing import List, Tuple


def py3round(x: float) -> int:
    """albumentations.augmentations.geometric.py3round (imported at predictor.py:12)."""
    if abs(round(x) - x) == 0.5:
        return int(2.0 * round(x / 2.0))
    return int(round(x))


def calculate_paddings(orig_h: int, orig_w: int) -> List[int]:
    """model_training/model/utils.py:71-77 -> [top, bottom, left, right]."""
    m = max(orig_h, orig_w)
    top, left = int((m - orig_h) / 2), int((m - orig_w) / 2)
    return [top, m - orig_h - top, left, m - orig_w - left]


def longest_max_size(h: int, w: int, size: int) -> Tuple[int, int, int, int]:
    """LongestMaxSize(size) then PadIfNeeded(size, size) of an h x w image -> (new_h, new_w, pad_top, pad_left), as
    FaceMeshPredictor._geometry computes it."""
    scale = size / float(max(h, w))
    new_h, new_w = py3round(h * scale), py3round(w * scale)
    pads = calculate_paddings(new_h, new_w)
    return new_h, new_w, pads[0], pads[2]
