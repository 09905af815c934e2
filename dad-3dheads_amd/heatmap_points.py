"""ctypes front of csrc/heatmap_points.hip: from the network's 2-D outputs to landmark points without a host wait.

    heatmap_peaks          `unravel_index` of the reference (model_training/model/utils.py:44-52): (k // H, k % H) of the argmax of
                           sigmoid(heatmap) (predictor.py:108-112) or of the values (train/flame_lightning_model.py:294-297)
    points_from_landmarks  predictor.py:132-133,147-152 on the regressed landmarks: * 256, clip, pads, scale, astype(int)
    points_from_heatmap    the same on `float(stride) * unravel_index(sigmoid(heatmap)).flip(-1)`: the peaks, then the readjustment

Device tensors only, and nothing here synchronises: the launches are queued on the current stream. There is no CPU fallback.
"""
from __future__ import annotations

from typing import Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib

_DTYPE = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16,
          torch.uint8: _lib.HEATMAP_DTYPE_U8}
Geometry = Union[Tuple[float, float, float], Sequence[Tuple[float, float, float]], Tensor]


def heatmap_peaks(heatmap: Tensor, sigmoid: bool = False, return_peak: bool = False):
    """int32 CUDA `[B,C,2]` (row, col) = (k // H, k % H) with k = torch.argmax over each `[H,W]` plane of `heatmap` (`[B,C,H,W]`,
    float32 / float16 / bfloat16 / uint8), resp. of `torch.sigmoid(heatmap)` in the heatmap's dtype with `sigmoid=True`. A
    contiguous or a channels-last tensor is read where it lies; any other is made contiguous first. With `return_peak` also the
    winning values, float32 `[B,C]`."""
    if heatmap.ndim != 4 or not heatmap.is_cuda or heatmap.dtype not in _DTYPE:
        raise ValueError(f"expected a CUDA [B,C,H,W] heatmap of float32, float16, bfloat16 or uint8, got {heatmap.dtype} "
                         f"{tuple(heatmap.shape)} on {heatmap.device}")
    hm = heatmap.detach()
    if hm.is_contiguous():
        layout = _lib.LAYOUT_NCHW
    elif hm.is_contiguous(memory_format=torch.channels_last):
        layout = _lib.LAYOUT_NHWC
    else:
        hm, layout = hm.contiguous(), _lib.LAYOUT_NCHW
    b, c, h, w = hm.shape
    dev = hm.device
    yx = torch.empty((b, c, 2), dtype=torch.int32, device=dev)
    peak = torch.empty((b, c), dtype=torch.float32, device=dev) if return_peak else None
    if b * c > 0:  # an empty plane is the C side's refusal
        _lib.check(_lib.load().dad3d_heatmap_argmax(hm.data_ptr(), _DTYPE[hm.dtype], b, c, h, w, layout, int(bool(sigmoid)), yx.data_ptr(),
                                                    None if peak is None else peak.data_ptr(), dev.index or 0,
                                                    torch.cuda.current_stream(dev).cuda_stream))
    return (yx, peak) if return_peak else yx


def _readjust(src: Tensor, kind: int, mul: float, limit: float, geometry: Geometry) -> Tensor:
    b, n = src.shape[0], src.shape[1]
    dev = src.device
    out = torch.empty((b, n, 2), dtype=torch.int32, device=dev)
    if b * n == 0:
        return out
    geo, triple = None, (0, 0, 1.0)
    if torch.is_tensor(geometry):
        geo = geometry.to(dev, torch.float64).contiguous()
    elif len(geometry) == 3 and not hasattr(geometry[0], "__len__"):
        triple = (int(geometry[0]), int(geometry[1]), float(geometry[2]))
    else:  # a list of triples: one upload
        geo = torch.tensor([[float(g[0]), float(g[1]), float(g[2])] for g in geometry], dtype=torch.float64).to(dev, non_blocking=True)
    if geo is not None and tuple(geo.shape) == (b, 5):  # a crop's points in its frame: + (x, y) after the truncation
        _lib.check(_lib.load().dad3d_points_readjust_frame(src.data_ptr(), kind, b, n, float(mul), float(limit), geo.data_ptr(), out.data_ptr(),
                                                           dev.index or 0, torch.cuda.current_stream(dev).cuda_stream))
        return out
    if geo is not None and tuple(geo.shape) != (b, 3):
        raise ValueError(f"expected one (pad_left, pad_top, scale) triple, {b} of them or {b} rows (pad_left, pad_top, scale, x, y), "
                         f"got {tuple(geo.shape)}")
    _lib.check(_lib.load().dad3d_points_readjust(src.data_ptr(), kind, b, n, float(mul), float(limit), None if geo is None else geo.data_ptr(),
                                                 triple[0], triple[1], triple[2], out.data_ptr(), dev.index or 0,
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return out


def points_from_landmarks(lm: Tensor, geometry: Geometry, img_size: int) -> Tensor:
    """int32 CUDA `[B,n,2]`: `((lm * 256.0).clip(0, img_size) - (pad_left, pad_top)) / scale` truncated, as numpy evaluates it on
    the float32 landmarks `[B, 2n]` or `[B,n,2]` (predictor.py:132-133,147-152). `geometry` is one (pad_left, pad_top, scale)
    triple for the batch, a list of one per image, or a float64 `[B,3]` tensor; the scale is `img_size / float(max_side)`. A float64
    `[B,5]` tensor (pad_left, pad_top, scale, x, y) is the geometry of crops (`dad3d_preprocess_boxes`): the integers (x, y), the
    crop's origin in its frame, are added after the truncation."""
    if not lm.is_cuda or lm.ndim not in (2, 3) or lm.shape[-1] % 2:
        raise ValueError(f"expected CUDA landmarks [B,2n] or [B,n,2], got {tuple(lm.shape)} on {lm.device}")
    src = lm.detach().to(torch.float32).reshape(lm.shape[0], -1, 2).contiguous()
    return _readjust(src, _lib.POINTS_SRC_XY_F32, 256.0, float(img_size), geometry)


def points_from_heatmap(heatmap: Tensor, geometry: Geometry, img_size: int, stride: int, sigmoid: bool = True) -> Tensor:
    """int32 CUDA `[B,C,2]`: `points_from_landmarks`' arithmetic on `float(stride) * heatmap_peaks(heatmap, sigmoid).flip(-1)`
    (predictor.py:108-112): the peaks, then the readjustment with the flip folded in."""
    return _readjust(heatmap_peaks(heatmap, sigmoid=sigmoid), _lib.POINTS_SRC_YX_I32, float(stride), float(img_size), geometry)
