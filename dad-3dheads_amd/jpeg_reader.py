"""`PIL.Image.open` for baseline JPEG files with the work done on the MI355X (csrc/jpeg_decode.hip), bit-equal to
PIL (libjpeg-turbo): Huffman-coded sequential files with one scan, grey or YCbCr at 4:4:4, 4:2:2 or 4:2:0, with or without restart
markers.

`JpegDecoder().decode(sources)` walks the marker segments of every file up to SOF on the host (to size the outputs), copies the
files to the device in one transfer and decodes them there in one set of launches, whatever their sizes: marker walk and tables,
entropy decode (one lane per restart segment, so one lane per file without restart markers), IDCT, upsampling, colour.
`JpegDecoder(entropy="sync")` takes the second entropy stage (csrc/jpeg_decode_sync.hip): a file without restart
markers is cut into pieces of `piece_bytes` that are decoded side by side, and what it gives is accepted only where it is provably
the serial result; the pixels and the flags are the same. The device decodes only what it has fully checked. An item it flags -- a valid file outside the decoder (progressive, arithmetic coding, CMYK,
other sampling factors, ...) or a damaged one -- is decoded by PIL on the host and uploaded, so the pixels are PIL's, and what PIL
refuses raises PIL's own error.

Packing, `decode` / `decode_packed`, their launch sequence and the read-back of the flags are `_packed_files.PackedDecoder`'s, shared
with `png_reader`; here is what is JPEG's own: the walk to SOF, the heads of a packed buffer, the two entropy stages' library calls.
"""
from __future__ import annotations

import io
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._packed_files import DecodedImages, PackedDecoder, Source

SOI = b"\xff\xd8"
_MODE = {1: "L", 3: "RGB"}
_MAX_BLOCKS = 1 << 22  # csrc/jpeg_entropy.hpp: a larger file goes to PIL
_HEAD_BYTES = 1 << 16  # what `decode_packed` asks a buffer on the device for per file: SOF lies behind the APPn segments
ENTROPY = ("segments", "sync")
SYNC_PIECE_BYTES = 128  # the default of entropy="sync": the fastest of 64 / 128 / 256 in tests/perf/bench_jpeg_decode_sync.py


def _pil_decode(data: bytes, channels: Optional[int]) -> np.ndarray:
    """uint8 [H,W,C] as PIL decodes the file; `channels` -> `convert` to L / RGB. Raises PIL's error for a bad file. With
    `channels=None` a file that PIL opens in another mode than L or RGB (CMYK) has no form of its own here and is refused."""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.load()
    if channels is not None:
        if im.mode != _MODE[channels]:
            im = im.convert(_MODE[channels])
    elif im.mode not in _MODE.values():
        raise ValueError(f"a JPEG of PIL mode {im.mode}: pass channels=1 or 3 for PIL's conversion")
    arr = np.asarray(im)
    return np.ascontiguousarray(arr[:, :, None] if arr.ndim == 2 else arr)


def _header(data: bytes):
    """(height, width, components) from the first SOF0, or None where the host cannot size an output: PIL gets such a file."""
    return _header_of(data, len(data))


def _header_of(data: bytes, size: int):
    """`_header` from the first bytes of a file of `size` bytes: the marker segments up to SOF, nothing else."""
    if size < 4 or size >= 2 ** 31 or data[:2] != SOI:
        return None
    pos, n = 2, len(data)
    while pos + 4 <= n and data[pos] == 0xFF:
        marker, seg = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        if seg < 2:
            return None
        if marker == 0xC0:
            if seg < 8 or pos + 10 > n:
                return None
            h, w, comps = data[pos + 5] << 8 | data[pos + 6], data[pos + 7] << 8 | data[pos + 8], data[pos + 9]
            if data[pos + 4] != 8 or h < 1 or w < 1 or comps not in (1, 3) or comps * ((w + 7) // 8 + 1) * ((h + 7) // 8 + 1) > _MAX_BLOCKS:
                return None
            return h, w, comps
        if not (0xE0 <= marker <= 0xEF or marker in (0xFE, 0xDB, 0xC4, 0xDD)):
            return None  # another SOF, SOS without a frame, anything this reader does not know
        pos += 2 + seg
    return None


class JpegImages(DecodedImages):
    """The result of `JpegDecoder.decode`: `DecodedImages` (the flags are `_lib.JPEG_DECODE_FLAG_*`), and `.modes` int32 per file,
    how its entropy data was decoded: `_lib.JPEG_DECODE_SYNC_MODE_*` (0 one lane per restart segment, 1 in verified pieces, 2 serially
    because not verified), -1 for a file that never reached the device or that PIL decoded."""

    def __init__(self, images: List[Tensor], flags: np.ndarray, modes: Optional[np.ndarray] = None):
        super().__init__(images, flags)
        self.modes = np.full(len(images), -1, dtype=np.int32) if modes is None else modes


class JpegDecoder(PackedDecoder):
    """`decode(sources, channels=None)` and `decode_packed(buffer, offsets, sizes, channels=None, heads=None)` of
    `_packed_files.PackedDecoder`: `channels` 1 grey, 3 colour. A buffer on the CPU is walked up to SOF file by file; a buffer on
    the device is asked for the first 64 KB of every file, and a file whose SOF lies behind them goes to PIL. With entropy="sync"
    the modes come back beside the flags, as info words [n, 4]."""

    _MODE = _MODE
    _header = staticmethod(_header)
    _pil_decode = staticmethod(_pil_decode)

    def __init__(self, device: Optional[Union[int, torch.device]] = None, entropy: str = "segments", piece_bytes: Optional[int] = None):
        """`entropy`: "segments" one lane per restart segment; "sync" a file without restart markers in pieces of `piece_bytes` (a
        power of two, 16 .. 256; None: SYNC_PIECE_BYTES)."""
        if entropy not in ENTROPY:
            raise ValueError(f"entropy must be one of {ENTROPY}, got {entropy!r}")
        if piece_bytes is None:
            piece_bytes = SYNC_PIECE_BYTES
        if piece_bytes not in (16, 32, 64, 128, 256):
            raise ValueError(f"piece_bytes must be a power of two in 16 .. 256, got {piece_bytes}")
        self.entropy, self.piece_bytes = entropy, int(piece_bytes)
        self._INFO = (4,) if entropy == "sync" else None
        super().__init__(device)

    def _heads_of(self, buffer: Tensor, offsets: List[int], sizes: List[int]) -> list:
        if buffer.device.type == "cpu":
            view = buffer.numpy()
            return [_header_of(view[o:o + z].tobytes(), z) if z else None for o, z in zip(offsets, sizes)]
        return [_header_of(buffer[o:o + min(z, _HEAD_BYTES)].cpu().numpy().tobytes(), z) if z else None for o, z in zip(offsets, sizes)]

    def _plan(self, rows: list):
        desc = np.asarray(rows, dtype=np.int64)
        if self.entropy == "sync":  # behind the rows, four columns a file for its piece and group tables
            desc = np.concatenate([desc.ravel(), np.zeros(len(rows) * (_lib.JPEG_DECODE_SYNC_DESC_INTS - _lib.JPEG_DECODE_DESC_INTS), np.int64)])
            grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, dtype=np.int32)
            return desc, self._lib.dad3d_jpeg_decode_sync_scratch_bytes(desc.ctypes.data, len(rows), grid.ctypes.data, self.piece_bytes), grid
        grid = np.zeros(_lib.JPEG_DECODE_GRID_INTS, dtype=np.int32)
        return desc, self._lib.dad3d_jpeg_decode_scratch_bytes(desc.ctypes.data, len(rows), grid.ctypes.data), grid

    def _run(self, grid, data, desc, n, out, flags, info, scratch, index, stream) -> int:
        if self.entropy == "sync":
            return self._lib.dad3d_jpeg_decode_sync(data.data_ptr(), data.numel(), desc.data_ptr(), n, grid.ctypes.data, self.piece_bytes,
                                                    out.data_ptr(), out.numel(), flags.data_ptr(), info.data_ptr(), scratch.data_ptr(),
                                                    scratch.numel(), index, stream)
        return self._lib.dad3d_jpeg_decode(data.data_ptr(), data.numel(), desc.data_ptr(), n, grid.ctypes.data, out.data_ptr(), out.numel(),
                                           flags.data_ptr(), scratch.data_ptr(), scratch.numel(), index, stream)

    def _result(self, images, flags, on_device, got_flags, got_info) -> JpegImages:
        modes = np.full(len(images), -1, dtype=np.int32)
        done = np.asarray(got_flags[:len(on_device)]) == 0
        modes[np.asarray(on_device, dtype=np.int64)[done]] = _lib.JPEG_DECODE_SYNC_MODE_SEGMENTS if got_info is None else got_info[done, 0]
        return JpegImages(images, flags, modes)


def load_jpeg_batch(sources: Sequence[Source], channels: Optional[int] = 3, device: Optional[Union[int, torch.device]] = None,
                    entropy: str = "segments") -> List[Tensor]:
    """One uint8 CUDA [H,W,channels] tensor per file: `np.asarray(Image.open(f).convert("RGB"))` for the default `channels=3`."""
    return JpegDecoder(device, entropy=entropy).decode(sources, channels).tensors()
