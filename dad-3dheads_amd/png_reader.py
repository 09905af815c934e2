"""`PIL.Image.open` and `zlib.decompress` with the work done on the MI355X (csrc/png_decode.hip): the inverse of
`writers.png_batch` / `writers.zlib_compress_batch`, and of any other PNG encoder's 8-bit grey, grey + alpha, RGB and RGBA files.

`PngDecoder().decode(sources)` reads the signature and IHDR of every file on the host (to size the outputs), copies the files to
the device in one transfer and decodes them there in one set of launches, whatever their sizes: chunk walk and CRCs, inflate (one
wave per IDAT for the files this library wrote, one wave per file otherwise), unfilter, channel conversion. The device decodes only
what it has fully checked. An item it flags -- a valid file outside the decoder (palette, 16-bit, 1 / 2 / 4-bit, Adam7) or a damaged
one -- is decoded by PIL on the host and uploaded, so the pixels are PIL's, and what PIL refuses raises PIL's own error.
"""
from __future__ import annotations

import ctypes as C
import io
import os
import struct
import zlib
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib

Source = Union[str, os.PathLike, bytes, bytearray, memoryview]
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}  # colour type -> channels
_MODE = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
_ALIGN = 16


def _align(n: int) -> int:
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def _bytes_of(source: Source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as f:
        return f.read()


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


class PngImages:
    """The result of `PngDecoder.decode`: `.tensors()` one uint8 CUDA [H,W,C] tensor per file; `.flags` the device's flag per file
    (int32 on the host: 0, or `_lib.PNG_DECODE_FLAG_*` for an item PIL decoded; -1 for a file that never reached the device);
    `.segmented` True where the per-IDAT path produced the file; `.shapes` [(H, W, C)]."""

    def __init__(self, images: List[Tensor], flags: np.ndarray, segmented: np.ndarray):
        self._images = images
        self.flags = flags
        self.segmented = segmented
        self.shapes = [tuple(t.shape) for t in images]

    def tensors(self) -> List[Tensor]:
        return list(self._images)

    def __len__(self) -> int:
        return len(self._images)


class PngDecoder:
    def __init__(self, device: Optional[Union[int, torch.device]] = None):
        _lib.require_gpu()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = _lib.load()

    def decode(self, sources: Sequence[Source], channels: Optional[int] = None, force_general: bool = False) -> PngImages:
        """`sources`: paths or bytes. `channels`: None keeps each file's own (1 grey, 2 grey + alpha, 3 RGB, 4 RGBA); 1 .. 4 converts
        as PIL's `convert` to L / LA / RGB / RGBA does. `force_general` sends every file through the serial inflate (for tests and
        the bench). One synchronisation: the flags. Packs the files the device will read into one pinned buffer (a file the host cannot size
        goes to PIL as it is), then `decode_packed`'s launches and finish."""
        pending = self._launch(sources, channels, force_general)
        return pending.finish(*pending.flags_on_host())

    def _launch(self, sources: Sequence[Source], channels: Optional[int] = None, force_general: bool = False) -> "_PendingDecode":
        """`decode` without its synchronisation: see `_launch_packed`."""
        if channels is not None and channels not in _MODE:
            raise ValueError(f"channels must be None or 1 .. 4, got {channels}")
        files = [_bytes_of(s) for s in sources]
        heads = [_header(f) for f in files]
        offsets, at = [], 0
        for f, head in zip(files, heads):  # only the files the device will read are staged: the others go to PIL as they are
            offsets.append(at)
            at += _align(len(f)) if head is not None else 0
        staged = torch.zeros(at, dtype=torch.uint8, pin_memory=True) if at else torch.zeros(0, dtype=torch.uint8)
        view = staged.numpy()
        for off, f, head in zip(offsets, files, heads):
            if head is not None:
                view[off:off + len(f)] = np.frombuffer(f, dtype=np.uint8)
        pending = self._launch_packed(staged, offsets, [len(f) if h is not None else 0 for f, h in zip(files, heads)], channels, force_general,
                                      heads)
        pending.unstaged = {i: f for i, (f, h) in enumerate(zip(files, heads)) if h is None}
        return pending

    def decode_packed(self, buffer: Tensor, offsets: Sequence[int], sizes: Sequence[int], channels: Optional[int] = None,
                      force_general: bool = False, heads: Optional[Sequence] = None) -> PngImages:
        """`decode` for files that already lie in one uint8 buffer, on the CPU (ideally pinned) or on the device: file i is
        buffer[offsets[i] : offsets[i] + sizes[i]], every offset a multiple of 16 and the buffer long enough to hold every file
        rounded up to 16 bytes (`_align`). `heads`: `_header` of every file where the caller has read it already; a buffer on the
        device is otherwise asked for its first 33 bytes per file. One synchronisation: the flags."""
        pending = self._launch_packed(buffer, offsets, sizes, channels, force_general, heads)
        return pending.finish(*pending.flags_on_host())

    def _launch_packed(self, buffer, offsets, sizes, channels, force_general=False, heads=None) -> "_PendingDecode":
        """The launches of `decode_packed` without its synchronisation: the caller reads `.dev_flags` / `.dev_info` (None when no file
        reached the device) back with whatever else it waits for and hands them to `.finish`."""
        if channels is not None and channels not in _MODE:
            raise ValueError(f"channels must be None or 1 .. 4, got {channels}")
        if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
            raise ValueError("decode_packed takes one contiguous uint8 buffer")
        offsets, sizes = [int(o) for o in offsets], [int(z) for z in sizes]
        n = len(sizes)
        if len(offsets) != n or any(o < 0 or z < 0 or o % _ALIGN or _align(o + z) > buffer.numel() for o, z in zip(offsets, sizes) if z):
            raise ValueError("decode_packed: every file starts at a multiple of 16 and lies, rounded up to 16 bytes, inside the buffer")
        if heads is None:
            if buffer.device.type == "cpu":
                view = buffer.numpy()
                heads = [_header_of(view[o:o + min(z, 33)].tobytes(), z) for o, z in zip(offsets, sizes)]
            else:
                index = torch.tensor([o + k for o, z in zip(offsets, sizes) for k in range(33) if z >= 33], dtype=torch.int64, device=buffer.device)
                got, heads, at = buffer[index].cpu().numpy().tobytes(), [], 0
                for z in sizes:
                    heads.append(_header_of(got[at:at + 33], z) if z >= 33 else None)
                    at += 33 if z >= 33 else 0
        heads = [None if h is None else tuple(int(v) for v in h) for h in heads]
        pending = _PendingDecode(self, buffer, offsets, sizes, channels, heads)
        on_device = pending.on_device
        if on_device:
            dev = self.device
            index = torch.cuda.current_device() if dev.index is None else dev.index
            rows, out_at = [], 0
            for i in on_device:
                h, w, c = heads[i]
                oc = c if channels is None else channels
                rows.append([offsets[i], sizes[i], h, w, c, out_at, w * oc, oc, 0, 0, 0, 0])
                out_at += _align(h * w * oc)
            desc = np.asarray(rows, dtype=np.int64)
            most = C.c_int32(0)
            scratch_bytes = self._lib.dad3d_png_decode_scratch_bytes(desc.ctypes.data, len(rows), C.addressof(most))
            if scratch_bytes == 0:
                raise _lib.Dad3dError(_lib.E_INVALID, "dad3d_png_decode_scratch_bytes refused the batch")
            data = buffer.to(dev, non_blocking=True)  # one H2D transfer (none for a buffer on the device)
            desc_dev = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)  # from pinned memory: the host does not wait
            out = torch.empty(out_at, dtype=torch.uint8, device=dev)
            pending.dev_flags = torch.empty(len(rows), dtype=torch.int32, device=dev)
            pending.dev_info = torch.empty(len(rows), dtype=torch.int32, device=dev)
            scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
            _lib.check(self._lib.dad3d_png_decode(data.data_ptr(), data.numel(), desc_dev.data_ptr(), len(rows), most.value, out.data_ptr(), out_at,
                                                  pending.dev_flags.data_ptr(), pending.dev_info.data_ptr(), scratch.data_ptr(), scratch_bytes,
                                                  int(force_general), index, torch.cuda.current_stream(dev).cuda_stream))
            pending.rows, pending.out, pending.data = rows, out, data
        return pending


class _PendingDecode:
    """A launched `decode_packed`: the device's flags are still to be read."""

    def __init__(self, decoder: PngDecoder, buffer: Tensor, offsets: List[int], sizes: List[int], channels: Optional[int], heads: list):
        self.decoder, self.buffer, self.offsets, self.sizes, self.channels, self.heads = decoder, buffer, offsets, sizes, channels, heads
        self.on_device = [i for i in range(len(sizes)) if heads[i] is not None]
        self.dev_flags = self.dev_info = self.rows = self.out = self.data = None
        self.unstaged = {}  # index -> bytes of a file that is not in the buffer

    def flags_on_host(self):
        if not self.on_device:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        got = torch.stack([self.dev_flags, self.dev_info]).cpu().numpy()  # the sync
        return got[0], got[1]

    def file_bytes(self, i: int) -> bytes:
        if i in self.unstaged:
            return self.unstaged[i]
        return self.buffer[self.offsets[i]:self.offsets[i] + self.sizes[i]].cpu().numpy().tobytes()

    def finish(self, got_flags: np.ndarray, got_info: np.ndarray) -> PngImages:
        n = len(self.sizes)
        images: List[Optional[Tensor]] = [None] * n
        flags = np.full(n, -1, dtype=np.int32)
        segmented = np.zeros(n, dtype=bool)
        for k, i in enumerate(self.on_device):
            row = self.rows[k]
            flags[i] = got_flags[k]
            segmented[i] = bool(got_info[k] & _lib.PNG_DECODE_INFO_SEGMENTED)
            if got_flags[k] == 0:
                images[i] = self.out[row[5]:row[5] + row[2] * row[6]].view(row[2], row[3], row[7])
        for i in range(n):
            if images[i] is None:  # never silent data: PIL's pixels, or PIL's error
                images[i] = torch.from_numpy(np.array(_pil_decode(self.file_bytes(i), self.channels))).to(self.decoder.device)
        return PngImages(images, flags, segmented)


def load_png_batch(sources: Sequence[Source], channels: Optional[int] = 3, device: Optional[Union[int, torch.device]] = None) -> List[Tensor]:
    """One uint8 CUDA [H,W,channels] tensor per file: `np.asarray(Image.open(f).convert("RGB"))` for the default `channels=3`."""
    return PngDecoder(device).decode(sources, channels).tensors()


def zlib_decompress_batch(streams: Sequence[bytes], max_bytes: Union[int, Sequence[int]], device: Optional[Union[int, torch.device]] = None) -> List[bytes]:
    """`[zlib.decompress(s) for s in streams]`, inflated on the device: the inverse of `writers.zlib_compress_batch`. `max_bytes`: the
    room for each result (one number for all, or one per stream). A stream the device flags (damaged, or larger than its room) goes
    through `zlib.decompress`, which raises `zlib.error` for a damaged one."""
    _lib.require_gpu()
    lib = _lib.load()
    if device is None:
        device = torch.cuda.current_device()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    index = torch.cuda.current_device() if dev.index is None else dev.index
    streams = [bytes(s) for s in streams]
    if not streams:
        return []
    caps = [int(max_bytes)] * len(streams) if isinstance(max_bytes, int) else [int(m) for m in max_bytes]
    if len(caps) != len(streams) or min(caps) < 0:
        raise ValueError("max_bytes: one non-negative number, or one per stream")
    rows, at, out_at = [], 0, 0
    for s, cap in zip(streams, caps):
        rows.append([at, len(s), out_at, cap])
        at += _align(len(s))
        out_at += _align(cap)
    staged = torch.zeros(max(at, _ALIGN), dtype=torch.uint8, pin_memory=True)
    view = staged.numpy()
    for row, s in zip(rows, streams):
        view[row[0]:row[0] + row[1]] = np.frombuffer(s, dtype=np.uint8)
    data = staged.to(dev, non_blocking=True)
    desc = torch.tensor(rows, dtype=torch.int64).to(dev)
    out = torch.empty(max(out_at, _ALIGN), dtype=torch.uint8, device=dev)
    lengths = torch.empty(len(rows), dtype=torch.int64, device=dev)
    flags = torch.empty(len(rows), dtype=torch.int32, device=dev)
    _lib.check(lib.dad3d_zlib_decompress(data.data_ptr(), data.numel(), desc.data_ptr(), len(rows), out.data_ptr(), out.numel(),
                                         lengths.data_ptr(), flags.data_ptr(), index, torch.cuda.current_stream(dev).cuda_stream))
    host, ln, fl = out.cpu().numpy(), lengths.cpu().tolist(), flags.cpu().tolist()
    return [host[row[2]:row[2] + ln[k]].tobytes() if fl[k] == 0 else zlib.decompress(streams[k]) for k, row in enumerate(rows)]
