"""`PIL.Image.open` and `zlib.decompress` with the work done on the MI355X (csrc/png_decode.hip): the inverse of
`writers.png_batch` / `writers.zlib_compress_batch`, and of any other PNG encoder's 8-bit grey, grey + alpha, RGB and RGBA files.

`PngDecoder().decode(sources)` reads the signature and IHDR of every file on the host (to size the outputs), copies the files to
the device in one transfer and decodes them there in one set of launches, whatever their sizes: chunk walk and CRCs, inflate (one
wave per IDAT for the files this library wrote, one wave per file otherwise), unfilter, channel conversion. The device decodes only
what it has fully checked. An item it flags -- a valid file outside the decoder (palette, 16-bit, 1 / 2 / 4-bit, Adam7) or a damaged
one -- is decoded by PIL on the host and uploaded, so the pixels are PIL's, and what PIL refuses raises PIL's own error.

Packing, `decode` / `decode_packed`, their launch sequence and the read-back of the flags are `_packed_files.PackedDecoder`'s, shared
with `jpeg_reader`; here is what is PNG's own: the IHDR, the heads of a packed buffer, the library calls, PIL's conversions.
"""
from __future__ import annotations

import ctypes as C
import io
import struct
import zlib
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._packed_files import ALIGN, DecodedImages, PackedDecoder, Source, align, cuda_device, device_index, pack
from ._packed_files import align as _align, bytes_of as _bytes_of  # noqa: F401 -- the names callers know them by

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}  # colour type -> channels
_MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
_HEAD_BYTES = 33  # signature, IHDR


def _pil_decode(data: bytes, channels: Optional[int]) -> np.ndarray:
    """uint8 [H,W,C] as PIL decodes the file; `channels` -> `convert` to L / LA / RGB / RGBA. Raises PIL's error for a bad file.
    With `channels=None` a palette file comes back as RGB (RGBA where it has a tRNS chunk) and a bilevel one as L, which lose
    nothing; a file deeper than 8 bits has no uint8 form of its own (`convert` clamps it), so it is refused unless the caller
    asks for a channel count and with it for PIL's conversion."""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.load()
    if channels is not None:
        if im.mode != _MODE[channels]:
            im = im.convert(_MODE[channels])
    elif im.mode == "P":
        im = im.convert("RGBA" if "transparency" in im.info else "RGB")
    elif im.mode == "1":
        im = im.convert("L")
    elif im.mode not in _MODE.values():
        raise ValueError(f"a PNG of PIL mode {im.mode} does not fit uint8: pass channels=1 .. 4 for PIL's conversion")
    arr = np.asarray(im)
    return np.ascontiguousarray(arr[:, :, None] if arr.ndim == 2 else arr)


def _header(data: bytes):
    """(height, width, channels as the IHDR states them) or None where the host cannot size an output: PIL gets such a file."""
    return _header_of(data[:33], len(data))


def _header_of(data: bytes, size: int):
    """`_header` from the first 33 bytes of a file of `size` bytes."""
    if size < 33 or len(data) < 33 or data[:8] != SIGNATURE or data[12:16] != b"IHDR":
        return None
    w, h, depth, colour = struct.unpack(">IIBB", data[16:26])
    if depth != 8 or colour not in _CHANNELS or w < 1 or h < 1:
        return None
    c = _CHANNELS[colour]
    if w * 4 >= 2 ** 31 or h * (1 + w * c) >= 2 ** 31 or size >= 2 ** 31:
        return None
    return h, w, c


class PngImages(DecodedImages):
    """The result of `PngDecoder.decode`: `DecodedImages` (the flags are `_lib.PNG_DECODE_FLAG_*`), and `.segmented` True where the
    per-IDAT path produced the file."""

    def __init__(self, images: List[Tensor], flags: np.ndarray, segmented: np.ndarray):
        super().__init__(images, flags)
        self.segmented = segmented


class PngDecoder(PackedDecoder):
    """`decode(sources, channels=None, force_general=False)` and `decode_packed(buffer, offsets, sizes, channels=None,
    force_general=False, heads=None)` of `_packed_files.PackedDecoder`: `channels` 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA;
    `force_general` sends every file through the serial inflate (for tests and the bench). A buffer on the device is asked for the
    first 33 bytes of every file in one gather and one copy back."""

    _MODE = _MODE
    _INFO = ()  # one info word per file
    _header = staticmethod(_header)
    _pil_decode = staticmethod(_pil_decode)

    _OPTIONS = ("force_general",)

    def decode(self, sources: Sequence[Source], channels: Optional[int] = None, force_general: bool = False) -> PngImages:
        return super().decode(sources, channels, force_general=force_general)

    def _launch(self, sources: Sequence[Source], channels: Optional[int] = None, force_general: bool = False):
        return super()._launch(sources, channels, force_general=force_general)

    def decode_packed(self, buffer: Tensor, offsets: Sequence[int], sizes: Sequence[int], channels: Optional[int] = None,
                      force_general: bool = False, heads: Optional[Sequence] = None) -> PngImages:
        return super().decode_packed(buffer, offsets, sizes, channels, heads=heads, force_general=force_general)

    def _launch_packed(self, buffer, offsets, sizes, channels=None, force_general=False, heads=None):
        return super()._launch_packed(buffer, offsets, sizes, channels, heads=heads, force_general=force_general)

    def _heads_of(self, buffer: Tensor, offsets: List[int], sizes: List[int]) -> list:
        if buffer.device.type == "cpu":
            view = buffer.numpy()
            return [_header_of(view[o:o + min(z, _HEAD_BYTES)].tobytes(), z) for o, z in zip(offsets, sizes)]
        index = torch.tensor([o + k for o, z in zip(offsets, sizes) for k in range(_HEAD_BYTES) if z >= _HEAD_BYTES], dtype=torch.int64,
                             device=buffer.device)
        got, heads, at = buffer[index].cpu().numpy().tobytes(), [], 0
        for z in sizes:
            heads.append(_header_of(got[at:at + _HEAD_BYTES], z) if z >= _HEAD_BYTES else None)
            at += _HEAD_BYTES if z >= _HEAD_BYTES else 0
        return heads

    def _plan(self, rows: list, force_general: bool = False):
        desc, most = np.asarray(rows, dtype=np.int64), C.c_int32(0)
        return desc, self._lib.dad3d_png_decode_scratch_bytes(desc.ctypes.data, len(rows), C.addressof(most)), most.value

    def _run(self, most, data, desc, n, out, flags, info, scratch, index, stream, force_general: bool = False) -> int:
        return self._lib.dad3d_png_decode(data.data_ptr(), data.numel(), desc.data_ptr(), n, most, out.data_ptr(), out.numel(), flags.data_ptr(),
                                          info.data_ptr(), scratch.data_ptr(), scratch.numel(), int(force_general), index, stream)

    def _result(self, images, flags, on_device, got_flags, got_info) -> PngImages:
        segmented = np.zeros(len(images), dtype=bool)
        if on_device:
            segmented[on_device] = (np.asarray(got_info[:len(on_device)]) & _lib.PNG_DECODE_INFO_SEGMENTED) != 0
        return PngImages(images, flags, segmented)


def load_png_batch(sources: Sequence[Source], channels: Optional[int] = 3, device: Optional[Union[int, torch.device]] = None) -> List[Tensor]:
    """One uint8 CUDA [H,W,channels] tensor per file: `np.asarray(Image.open(f).convert("RGB"))` for the default `channels=3`."""
    return PngDecoder(device).decode(sources, channels).tensors()


def zlib_decompress_batch(streams: Sequence[bytes], max_bytes: Union[int, Sequence[int]], device: Optional[Union[int, torch.device]] = None) -> List[bytes]:
    """`[zlib.decompress(s) for s in streams]`, inflated on the device: the inverse of `writers.zlib_compress_batch`. `max_bytes`: the
    room for each result (one number for all, or one per stream). A stream the device flags (damaged, or larger than its room) goes
    through `zlib.decompress`, which raises `zlib.error` for a damaged one."""
    dev = cuda_device(device)
    lib = _lib.load()
    streams = [bytes(s) for s in streams]
    if not streams:
        return []
    caps = [int(max_bytes)] * len(streams) if isinstance(max_bytes, int) else [int(m) for m in max_bytes]
    if len(caps) != len(streams) or min(caps) < 0:
        raise ValueError("max_bytes: one non-negative number, or one per stream")
    staged, table = pack(streams, pinned=True, min_bytes=ALIGN)
    rows, out_at = [], 0
    for (at, size), cap in zip(table.tolist(), caps):
        rows.append([at, size, out_at, cap])
        out_at += align(cap)
    data = staged.to(dev, non_blocking=True)
    desc = torch.tensor(rows, dtype=torch.int64).to(dev)
    out = torch.empty(max(out_at, ALIGN), dtype=torch.uint8, device=dev)
    lengths = torch.empty(len(rows), dtype=torch.int64, device=dev)
    flags = torch.empty(len(rows), dtype=torch.int32, device=dev)
    _lib.check(lib.dad3d_zlib_decompress(data.data_ptr(), data.numel(), desc.data_ptr(), len(rows), out.data_ptr(), out.numel(),
                                         lengths.data_ptr(), flags.data_ptr(), device_index(dev), torch.cuda.current_stream(dev).cuda_stream))
    host, ln, fl = out.cpu().numpy(), lengths.cpu().tolist(), flags.cpu().tolist()
    return [host[row[2]:row[2] + ln[k]].tobytes() if fl[k] == 0 else zlib.decompress(streams[k]) for k, row in enumerate(rows)]
