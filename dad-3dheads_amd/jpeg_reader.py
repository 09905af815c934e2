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
"""
from __future__ import annotations

import ctypes as C
import io
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .png_reader import _ALIGN, Source, _align, _bytes_of

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


class JpegImages:
    """The result of `JpegDecoder.decode`: `.tensors()` one uint8 CUDA [H,W,C] tensor per file; `.flags` the device's flag per file
    (int32 on the host: 0, or `_lib.JPEG_DECODE_FLAG_*` for an item PIL decoded; -1 for a file that never reached the device);
    `.shapes` [(H, W, C)]; `.modes` int32 per file, how its entropy data was decoded: `_lib.JPEG_DECODE_SYNC_MODE_*` (0 one lane per
    restart segment, 1 in verified pieces, 2 serially because not verified), -1 for a file that never reached the device or that PIL
    decoded."""

    def __init__(self, images: List[Tensor], flags: np.ndarray, modes: Optional[np.ndarray] = None):
        self._images = images
        self.flags = flags
        self.modes = np.full(len(images), -1, dtype=np.int32) if modes is None else modes
        self.shapes = [tuple(t.shape) for t in images]

    def tensors(self) -> List[Tensor]:
        return list(self._images)

    def __len__(self) -> int:
        return len(self._images)


class JpegDecoder:
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
        _lib.require_gpu()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = _lib.load()

    def decode(self, sources: Sequence[Source], channels: Optional[int] = None) -> JpegImages:
        """`sources`: paths or bytes. `channels`: None keeps each file's own (1 grey, 3 colour); 1 and 3 convert as PIL's `convert`
        to L / RGB does. One synchronisation: the flags (and, with entropy="sync", the modes beside them)."""
        pending = self._launch(sources, channels)
        return pending.finish(*pending.words_on_host())

    def _launch(self, sources: Sequence[Source], channels: Optional[int]) -> "_PendingDecode":
        """Packs the files the device will read into one pinned buffer (a file the host cannot size goes to PIL as it is), then
        `_launch_packed`."""
        if channels is not None and channels not in _MODE:
            raise ValueError(f"channels must be None, 1 or 3, got {channels}")
        files = [_bytes_of(s) for s in sources]
        heads = [_header(f) for f in files]
        offsets, at = [], 0
        for f, head in zip(files, heads):
            offsets.append(at)
            at += _align(len(f)) if head is not None else 0
        staged = torch.zeros(at, dtype=torch.uint8, pin_memory=True) if at else torch.zeros(0, dtype=torch.uint8)
        view = staged.numpy()
        for off, f, head in zip(offsets, files, heads):
            if head is not None:
                view[off:off + len(f)] = np.frombuffer(f, dtype=np.uint8)
        pending = self._launch_packed(staged, offsets, [len(f) if h is not None else 0 for f, h in zip(files, heads)], channels, heads)
        pending.unstaged = {i: f for i, (f, h) in enumerate(zip(files, heads)) if h is None}
        return pending

    def decode_packed(self, buffer: Tensor, offsets: Sequence[int], sizes: Sequence[int], channels: Optional[int] = None,
                      heads: Optional[Sequence] = None) -> JpegImages:
        """`decode` for files that already lie in one uint8 buffer on the CPU (ideally pinned): file i is
        buffer[offsets[i] : offsets[i] + sizes[i]], every offset a multiple of 16 and the buffer long enough to hold every file
        rounded up to 16 bytes. `heads`: `_header` of every file where the caller has read it already; with them the buffer may lie
        on the device (a buffer there is otherwise asked for the first 64 KB of every file). One synchronisation: the flags."""
        pending = self._launch_packed(buffer, offsets, sizes, channels, heads)
        return pending.finish(*pending.words_on_host())

    def _launch_packed(self, buffer, offsets, sizes, channels, heads=None) -> "_PendingDecode":
        """The launches of `decode_packed` without its synchronisation: the caller reads `.dev_flags` (None when no file reached the
        device) back with whatever else it waits for and hands them to `.finish`, and with entropy="sync" `.dev_info` ([n][4]) too."""
        if channels is not None and channels not in _MODE:
            raise ValueError(f"channels must be None, 1 or 3, got {channels}")
        if not isinstance(buffer, Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
            raise ValueError("decode_packed takes one contiguous uint8 buffer")
        offsets, sizes = [int(o) for o in offsets], [int(z) for z in sizes]
        n = len(sizes)
        if len(offsets) != n or any(o < 0 or z < 0 or o % _ALIGN or _align(o + z) > buffer.numel() for o, z in zip(offsets, sizes) if z):
            raise ValueError("decode_packed: every file starts at a multiple of 16 and lies, rounded up to 16 bytes, inside the buffer")
        if heads is not None and len(heads) != n:
            raise ValueError("decode_packed: one head per file")
        if heads is None:
            if buffer.device.type == "cpu":
                view = buffer.numpy()
                heads = [_header_of(view[o:o + z].tobytes(), z) if z else None for o, z in zip(offsets, sizes)]
            else:
                heads = [_header_of(buffer[o:o + min(z, _HEAD_BYTES)].cpu().numpy().tobytes(), z) if z else None for o, z in zip(offsets, sizes)]
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
            sync = self.entropy == "sync"
            desc = np.asarray(rows, dtype=np.int64)
            if sync:  # behind the rows, four columns a file for its piece and group tables
                desc = np.concatenate([desc.ravel(), np.zeros(len(rows) * (_lib.JPEG_DECODE_SYNC_DESC_INTS - _lib.JPEG_DECODE_DESC_INTS), np.int64)])
                grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, dtype=np.int32)
                scratch_bytes = self._lib.dad3d_jpeg_decode_sync_scratch_bytes(desc.ctypes.data, len(rows), grid.ctypes.data, self.piece_bytes)
            else:
                grid = np.zeros(_lib.JPEG_DECODE_GRID_INTS, dtype=np.int32)
                scratch_bytes = self._lib.dad3d_jpeg_decode_scratch_bytes(desc.ctypes.data, len(rows), grid.ctypes.data)
            if scratch_bytes == 0:
                raise _lib.Dad3dError(_lib.E_INVALID, "dad3d_jpeg_decode_scratch_bytes refused the batch")
            data = buffer.to(dev, non_blocking=True)  # one H2D transfer (none for a buffer on the device)
            desc_dev = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)
            out = torch.empty(out_at, dtype=torch.uint8, device=dev)
            pending.dev_flags = torch.empty(len(rows), dtype=torch.int32, device=dev)
            scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if sync:
                pending.dev_info = torch.empty((len(rows), 4), dtype=torch.int32, device=dev)
                _lib.check(self._lib.dad3d_jpeg_decode_sync(data.data_ptr(), data.numel(), desc_dev.data_ptr(), len(rows), grid.ctypes.data,
                                                            self.piece_bytes, out.data_ptr(), out_at, pending.dev_flags.data_ptr(),
                                                            pending.dev_info.data_ptr(), scratch.data_ptr(), scratch_bytes, index, stream))
            else:
                _lib.check(self._lib.dad3d_jpeg_decode(data.data_ptr(), data.numel(), desc_dev.data_ptr(), len(rows), grid.ctypes.data,
                                                       out.data_ptr(), out_at, pending.dev_flags.data_ptr(), scratch.data_ptr(), scratch_bytes, index,
                                                       stream))
            pending.rows, pending.out, pending.data = rows, out, data
        return pending


class _PendingDecode:
    """A launched `decode_packed`: the device's flags are still to be read."""

    def __init__(self, decoder: JpegDecoder, buffer: Tensor, offsets: List[int], sizes: List[int], channels: Optional[int], heads: list):
        self.decoder, self.buffer, self.offsets, self.sizes, self.channels, self.heads = decoder, buffer, offsets, sizes, channels, heads
        self.on_device = [i for i in range(len(sizes)) if heads[i] is not None and sizes[i]]
        self.dev_flags = self.dev_info = self.rows = self.out = self.data = None
        self.unstaged = {}  # index -> bytes of a file that is not in the buffer

    def flags_on_host(self) -> np.ndarray:
        if not self.on_device:
            return np.zeros(0, np.int32)
        return self.dev_flags.cpu().numpy()  # the sync

    def words(self) -> List[Tensor]:
        """What is to be read back, on the device: the flags [n], and with entropy="sync" the info [n * 4] behind them."""
        return [t.reshape(-1) for t in (self.dev_flags, self.dev_info) if t is not None]

    def split(self, got: np.ndarray):
        """(flags, info or None) from the words as they came back in one array."""
        n = len(self.on_device)
        return got[:n], (got[n:5 * n].reshape(n, 4) if self.dev_info is not None else None)

    def words_on_host(self):
        if self.dev_info is None:
            return self.flags_on_host(), None
        return self.split(torch.cat(self.words()).cpu().numpy())  # the sync

    def file_bytes(self, i: int) -> bytes:
        if i in self.unstaged:
            return self.unstaged[i]
        return self.buffer[self.offsets[i]:self.offsets[i] + self.sizes[i]].cpu().numpy().tobytes()

    def finish(self, got_flags: np.ndarray, got_info: Optional[np.ndarray] = None) -> JpegImages:
        n = len(self.sizes)
        images: List[Optional[Tensor]] = [None] * n
        flags = np.full(n, -1, dtype=np.int32)
        modes = np.full(n, -1, dtype=np.int32)
        for k, i in enumerate(self.on_device):
            row = self.rows[k]
            flags[i] = got_flags[k]
            if got_flags[k] == 0:
                images[i] = self.out[row[5]:row[5] + row[2] * row[6]].view(row[2], row[3], row[7])
                modes[i] = got_info[k, 0] if got_info is not None else _lib.JPEG_DECODE_SYNC_MODE_SEGMENTS
        for i in range(n):
            if images[i] is None:  # never silent data: PIL's pixels, or PIL's error
                images[i] = torch.from_numpy(np.array(_pil_decode(self.file_bytes(i), self.channels))).to(self.decoder.device)
        return JpegImages(images, flags, modes)


def load_jpeg_batch(sources: Sequence[Source], channels: Optional[int] = 3, device: Optional[Union[int, torch.device]] = None,
                    entropy: str = "segments") -> List[Tensor]:
    """One uint8 CUDA [H,W,channels] tensor per file: `np.asarray(Image.open(f).convert("RGB"))` for the default `channels=3`."""
    return JpegDecoder(device, entropy=entropy).decode(sources, channels).tensors()
