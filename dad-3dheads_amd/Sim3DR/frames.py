"""The frame table of `Mesh.rasterize_frames` / `Mesh.render_frames`: uint8 RGB frames of any sizes and row strides, described to
the kernels as int64 rows {address of the first byte, h, w, row stride in bytes} -- the format of `dad3d_preprocess_boxes`.

`frame_table` is pure host code (tensor metadata only; it works on CPU tensors too). `DeviceFrames` keeps the frames, the table and
its device copy together, so that a caller who draws into the same frames again -- or captures the call into a graph -- uploads the
table once.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _lib

TILE = 64  # the raster's screen tile edge


def _as_list(frames: Union[Tensor, Sequence[Tensor]]) -> List[Tensor]:
    if isinstance(frames, Tensor):
        if frames.ndim != 4:
            raise ValueError(f"frames: one tensor must be [B,H,W,3], got {tuple(frames.shape)}")
        return list(frames.unbind(0))
    return list(frames)


def frame_table(frames: Union[Tensor, Sequence[Tensor]]) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
    """frames: a list of uint8 tensors `[H,W,3]` (any sizes, any row strides, views included) or one `[B,H,W,3]` tensor ->
    (int64 `[M,4]` host table {data_ptr, H, W, row stride in bytes}, `[(H, W), ..]`). Raises ValueError for anything the kernels
    do not take: another dtype or channel count, a channel stride other than 1 or a column stride other than 3, rows that run
    backwards or overlap, an empty frame, a frame of more than 4096 tiles of 64 x 64 pixels, more than 65535 frames, or frames
    on different devices."""
    fl = _as_list(frames)
    if len(fl) > _lib.FRAME_MAX_COUNT:
        raise ValueError(f"frames: {len(fl)} frames, at most {_lib.FRAME_MAX_COUNT}")
    rows, shapes = [], []
    for i, t in enumerate(fl):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"frames[{i}]: expected a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError(f"frames[{i}]: expected [H,W,3], got {tuple(t.shape)}")
        if t.device != fl[0].device:
            raise ValueError(f"frames[{i}]: on {t.device}, frames[0] on {fl[0].device}")
        h, w = int(t.shape[0]), int(t.shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"frames[{i}]: empty frame {h} x {w}")
        tiles = -(-h // TILE) * -(-w // TILE)
        if tiles > _lib.FRAME_MAX_TILES:
            raise ValueError(f"frames[{i}]: {h} x {w} pixels are {tiles} tiles of {TILE} x {TILE}, at most {_lib.FRAME_MAX_TILES}")
        if t.stride(2) != 1 or (w > 1 and t.stride(1) != 3):
            raise ValueError(f"frames[{i}]: pixels must be 3 adjacent bytes, 3 bytes apart; strides {tuple(t.stride())}")
        stride = int(t.stride(0)) if h > 1 else 3 * w  # a single row has no stride to speak of
        if stride < 3 * w:
            raise ValueError(f"frames[{i}]: a row stride of {stride} bytes for rows of {3 * w}: rows run backwards or overlap")
        rows.append((t.data_ptr(), h, w, stride))
        shapes.append((h, w))
    return np.asarray(rows, dtype=np.int64).reshape(len(rows), 4), shapes


class DeviceFrames:
    """Frames with their table on the host and on the device. The frames are kept alive; the table holds their addresses."""

    def __init__(self, frames: Union[Tensor, Sequence[Tensor]], device: torch.device):
        self.source = frames
        self.frames = _as_list(frames)
        self.host, self.shapes = frame_table(self.frames)
        for i, t in enumerate(self.frames):
            if t.device != device:
                raise ValueError(f"frames[{i}]: on {t.device}, expected {device}")
        self.device = torch.from_numpy(self.host).to(device) if len(self.frames) else torch.empty((0, 4), dtype=torch.int64, device=device)

    def __len__(self) -> int:
        return len(self.frames)
