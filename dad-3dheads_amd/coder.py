"""The reference's heatmap target (`model_training/data/coder.py` `HeatmapCoder`, `draw_gaussian` of data/utils.py:37-71) on
the GPU.

Every channel holds at most one stamp, so the target is a (2r+1)^2 table placed into a zeroed channel. `stamp_table` builds
that table on the host with the reference's own expressions -- `gaussian_2d` in float64 with its `eps * max` cut, the float32
store of `np.maximum(..., out=)`, `np.uint8(255.0 * heatmap)` of flame_dataset.py:198 and `uint8 / 255.0` of mixins.py:50 --
and the kernel (csrc/train_objective.hip) only places it, so every form is byte-exact by construction.

Use `encode` in the training step, after the batch is on the GPU: it needs 35 KB of keypoints instead of the 17.8 MB of
uint8 heatmaps a B = 64 batch carries from the loader. `__call__` keeps the reference's per-item NumPy contract, but it runs
on the GPU: a forked DataLoader worker must not initialise HIP, so do not call it inside the loader. Use `dataset.FlameDataset`
(CPU-only items) with its collate and `dataset.FlameBatchBuilder`, which calls `encode` after the batch is on the device.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

__all__ = ["HeatmapCoder", "stamp_table", "floor_divide_f32", "FORMS"]

FORMS = {"raw": 0, "uint8": 1, "float": 2}  # DAD3D_HEATMAP_RAW / _UINT8 / _FLOAT


def _stamp(radius: Union[int, str]) -> Tuple[np.ndarray, int]:
    """draw_gaussian's kernel and radius (data/utils.py:37-54)."""
    if radius == "pointwise":
        return np.float32([[0.5, 0.75, 0.5], [0.75, 1.0, 0.75], [0.5, 0.75, 0.5]]), 1
    r = int(radius)
    if r != radius or r < 0:
        raise ValueError(f"radius must be a non-negative int or 'pointwise', not {radius!r}")
    diameter = 2 * r + 1
    sigma = diameter / 6
    m = n = int((diameter - 1.0) / 2.0)
    y, x = np.ogrid[-m: m + 1, -n: n + 1]
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h, r


def stamp_table(radius: Union[int, str], form: str = "raw") -> np.ndarray:
    """The (2r+1)^2 values one stamp writes into a zeroed channel, in `form`: "raw" (the coder's float32), "uint8" (the
    dataset's bytes) or "float" (get_input's uint8 / 255 as float32)."""
    if form not in FORMS:
        raise ValueError(f"form must be one of {sorted(FORMS)}, not {form!r}")
    g, _ = _stamp(radius)
    raw = np.zeros(g.shape, dtype=np.float32)
    np.maximum(raw, g * 1, out=raw)  # data/utils.py:70: the float32 heatmap takes max(0, gaussian * k), k = 1
    if form == "raw":
        return raw
    u8 = np.uint8(255.0 * raw)  # flame_dataset.py:198 (255.0 * float32 stays float32 under NumPy 2)
    if form == "uint8":
        return u8
    return u8.astype(np.float32) / np.float32(255.0)  # model/flame.py:232-236 uint8_to_float32: x.div(255.0), fp32


def floor_divide_f32(a: np.ndarray, b: float) -> np.ndarray:
    """numpy's float32 floor_divide restated (npy_divmodf): fmod first, then the quotient of the difference. The kernel
    applies the same rule; `np.floor(a / b)` differs from it for strides that are not powers of two."""
    a = np.asarray(a, dtype=np.float32)
    b = np.float32(b)
    with np.errstate(all="ignore"):
        mod = np.fmod(a, b)
        div = (a - mod) / b
        fix = (mod != 0) & ((b < 0) != (mod < 0))
        div = np.where(fix, div - np.float32(1), div).astype(np.float32)
        fl = np.floor(div)
        fl = np.where(div - fl > np.float32(0.5), fl + np.float32(1), fl).astype(np.float32)
        zero = np.copysign(np.float32(0), a / b).astype(np.float32)
        return np.where(div != 0, fl, zero).astype(np.float32)


class HeatmapCoder:
    """model_training/data/coder.py:7-24. `data_config` holds img_size, and optionally radius (5) and stride (2)."""

    def __init__(self, data_config: Dict[str, Any], num_classes: int, device: Optional[Union[int, torch.device]] = None) -> None:
        super().__init__()
        self.num_classes = num_classes
        self._img_size = data_config["img_size"]
        self._radius = data_config.get("radius", 5)
        self._stride = data_config.get("stride", 2)
        _stamp(self._radius)  # validate once
        self.size = int(self._img_size // self._stride)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device if isinstance(device, int) else device.index or 0))
        self._tables: Dict[str, Tensor] = {}
        self.invalid_points: Optional[Tensor] = None  # int32 [1] on the device: present points with a NaN / inf centre

    def _table(self, form: str) -> Tensor:
        if form not in self._tables:
            self._tables[form] = torch.from_numpy(np.ascontiguousarray(stamp_table(self._radius, form))).to(self.device)
        return self._tables[form]

    def encode(self, keypoints: Tensor, presence: Tensor, form: str = "uint8", strict: bool = False,
               out: Optional[Tensor] = None) -> Tensor:
        """[B,C,2] keypoints (resized-image pixels, read as float32) and [B,C] presence -> [B,C,S,S] heatmaps on the GPU, on
        the current stream. `form`: "uint8" (the dataset's bytes), "float" (what get_input makes of them) or "raw" (the
        coder's float32). A present point whose centre is NaN or inf -- the reference raises -- leaves its channel zero and
        is counted in `invalid_points`; `strict=True` waits for the count and raises the reference's ValueError instead."""
        from . import _lib

        if form not in FORMS:
            raise ValueError(f"form must be one of {sorted(FORMS)}, not {form!r}")
        if keypoints.ndim != 3 or keypoints.shape[2] != 2 or presence.shape != keypoints.shape[:2]:
            raise ValueError(f"expected [B,C,2] keypoints and [B,C] presence, got {tuple(keypoints.shape)} and {tuple(presence.shape)}")
        b, c = keypoints.shape[:2]
        if c > self.num_classes:
            raise IndexError(f"{c} keypoints for {self.num_classes} heatmap channels")
        kp = keypoints.detach().to(self.device, torch.float32)
        pr = presence.detach().to(self.device)
        pr = (pr if pr.dtype in (torch.bool, torch.uint8) else pr != 0).to(torch.uint8)
        if c < self.num_classes:  # the reference leaves the channels without a keypoint at zero
            kp = torch.cat([kp, kp.new_zeros((b, self.num_classes - c, 2))], 1)
            pr = torch.cat([pr, pr.new_zeros((b, self.num_classes - c))], 1)
        kp, pr = kp.contiguous(), pr.contiguous()
        dtype = torch.uint8 if form == "uint8" else torch.float32
        shape = (b, self.num_classes, self.size, self.size)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        elif out.shape != shape or out.dtype != dtype or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
        if strict:
            counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        else:
            if self.invalid_points is None:
                self.invalid_points = torch.zeros(1, dtype=torch.int32, device=self.device)
            counter = self.invalid_points
        radius = 1 if self._radius == "pointwise" else int(self._radius)
        _lib.check(_lib.load().dad3d_heatmap_encode(
            out.data_ptr(), FORMS[form], kp.data_ptr(), pr.data_ptr(), b, self.num_classes, float(np.float32(self._stride)),
            self.size, radius, self._table(form).data_ptr(), counter.data_ptr(), self.device.index or 0,
            torch.cuda.current_stream(self.device).cuda_stream))
        if strict and int(counter.item()) > 0:
            raise ValueError("cannot convert float NaN to integer")  # int(nan) in data/utils.py:56 (inf // stride is NaN too)
        return out

    def __call__(self, keypoints: np.ndarray, presence: np.ndarray) -> np.ndarray:
        """coder.py:17-24: one item's [C,S,S] float32 heatmap as a NumPy array (computed on the GPU, then copied back)."""
        kp = torch.from_numpy(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2))
        pr = torch.from_numpy(np.asarray(presence).reshape(-1).astype(bool))
        if pr.shape[0] < kp.shape[0]:
            raise IndexError(f"presence has {pr.shape[0]} entries for {kp.shape[0]} keypoints")
        pr = pr[: kp.shape[0]]
        return self.encode(kp[None], pr[None], form="raw", strict=True)[0].cpu().numpy()
