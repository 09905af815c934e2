"""Files packed in one buffer, and the decoder that reads them on the MI355X: what `png_reader` and `jpeg_reader` share (DESIGN.md
4.16, 4.19). One copy of the staging rule (every file at a multiple of 16 bytes, zeros between them), of `decode_packed`'s argument
checks, of the 12-column descriptor row, of the launch sequence and of the read-back of the flags. A format's reader keeps what is
its own: how a header sizes an output, how heads are fetched from a buffer, its library calls, its PIL fallback, its result class.
"""
from __future__ import annotations

import os
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib

Source = Union[str, os.PathLike, bytes, bytearray, memoryview]
ALIGN = 16


def align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def bytes_of(source: Source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as f:
        return f.read()


def cuda_device(device: Optional[Union[int, torch.device]] = None) -> torch.device:
    """`device` (None: the current one) as a torch.device; RuntimeError where no GPU is visible."""
    _lib.require_gpu()
    if device is None:
        device = torch.cuda.current_device()
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


def device_index(dev: torch.device) -> int:
    return torch.cuda.current_device() if dev.index is None else dev.index


def pack(items: Sequence[Any], pinned: bool = False, min_bytes: int = 0) -> Tuple[Tensor, np.ndarray]:
    """Byte strings or uint8 arrays -> (one zero-filled uint8 CPU buffer that holds item i at table[i, 0], a multiple of 16, the
    int64 table [n, 2] of (offset, size)). `pinned`: in pinned memory; `min_bytes`: the least length of the buffer."""
    arrays = [np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray, memoryview))
              else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in items]
    rows, at = [], 0
    for a in arrays:
        rows.append((at, a.size))
        at += align(a.size)
    at = max(at, int(min_bytes))
    buffer = torch.zeros(at, dtype=torch.uint8, pin_memory=bool(pinned and at))
    flat = buffer.numpy()
    for (off, size), a in zip(rows, arrays):
        flat[off:off + size] = a
    return buffer, np.asarray(rows, dtype=np.int64).reshape(-1, 2)


def check_packed(buffer: Any, offsets: Sequence[int], sizes: Sequence[int], heads: Optional[Sequence]) -> Tuple[List[int], List[int]]:
    """The contract of `decode_packed`, checked before anything is launched: (offsets, sizes) as lists of int, or ValueError."""
    if not isinstance(buffer, Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise ValueError("decode_packed takes one contiguous uint8 buffer")
    offsets, sizes = [int(o) for o in offsets], [int(z) for z in sizes]
    if len(offsets) != len(sizes) or any(o < 0 or z < 0 or o % ALIGN or align(o + z) > buffer.numel() for o, z in zip(offsets, sizes) if z):
        raise ValueError("decode_packed: every file starts at a multiple of 16 and lies, rounded up to 16 bytes, inside the buffer")
    if heads is not None and len(heads) != len(sizes):
        raise ValueError("decode_packed: one head per file")
    return offsets, sizes


def on_device(sizes: Sequence[int], heads: Sequence) -> List[int]:
    """The files the device reads: those the host could size and that hold a byte."""
    return [i for i in range(len(sizes)) if heads[i] is not None and sizes[i]]


def descriptor_rows(offsets: Sequence[int], sizes: Sequence[int], heads: Sequence, channels: Optional[int],
                    indices: Sequence[int]) -> Tuple[List[List[int]], int]:
    """(the library's rows [offset, size, h, w, c, out_at, row stride, out channels, 0, 0, 0, 0] of the files `indices`, the
    bytes of their outputs, each at a multiple of 16)."""
    rows, out_at = [], 0
    for i in indices:
        h, w, c = heads[i]
        oc = c if channels is None else channels
        rows.append([offsets[i], sizes[i], h, w, c, out_at, w * oc, oc, 0, 0, 0, 0])
        out_at += align(h * w * oc)
    return rows, out_at


def read_back(pendings: Sequence[Optional["PendingDecode"]], leading: Sequence[Tensor] = ()) -> Tuple[List[np.ndarray], List[Any]]:
    """The one wait for any number of launched decodes: their words, behind the int32 device tensors `leading`, come over in one
    copy. Returns (the values of `leading`, `(flags, info)` per pending as its `finish` takes them; None for a pending of None)."""
    words = [t.reshape(-1) for t in leading] + [w for p in pendings if p is not None for w in p.words()]
    if not words:
        got = np.zeros(0, np.int32)
    else:
        got = (words[0] if len(words) == 1 else torch.cat(words)).cpu().numpy()  # the sync
    cuts = np.cumsum([0] + [t.numel() for t in leading]).tolist()
    at, results = cuts[-1], []
    for p in pendings:
        n = 0 if p is None else sum(w.numel() for w in p.words())
        results.append(None if p is None else p.split(got[at:at + n]))
        at += n
    return [got[a:b] for a, b in zip(cuts, cuts[1:])], results


class DecodedImages:
    """`.tensors()` one uint8 CUDA [H,W,C] tensor per file; `.flags` the device's flag per file (int32 on the host: 0, or the
    format's `_lib.*_DECODE_FLAG_*` for an item PIL decoded; -1 for a file that never reached the device); `.shapes` [(H, W, C)]."""

    def __init__(self, images: List[Tensor], flags: np.ndarray):
        self._images = images
        self.flags = flags
        self.shapes = [tuple(t.shape) for t in images]

    def tensors(self) -> List[Tensor]:
        return list(self._images)

    def __len__(self) -> int:
        return len(self._images)


class PendingDecode:
    """A launched `decode_packed`: the device's words (`.dev_flags` [n], and `.dev_info` [n, ...] where the format has one; both
    None when no file reached the device) are still to be read."""

    def __init__(self, decoder: "PackedDecoder", buffer: Tensor, offsets: List[int], sizes: List[int], channels: Optional[int], heads: list):
        self.decoder, self.buffer, self.offsets, self.sizes, self.channels, self.heads = decoder, buffer, offsets, sizes, channels, heads
        self.on_device = on_device(sizes, heads)
        self.dev_flags = self.dev_info = self.rows = self.out = self.data = None
        self.unstaged = {}  # index -> bytes of a file that is not in the buffer

    def words(self) -> List[Tensor]:
        """What is to be read back, on the device: the flags [n], and the info words behind them."""
        return [t.reshape(-1) for t in (self.dev_flags, self.dev_info) if t is not None]

    def split(self, got: np.ndarray):
        """(flags, info or None) from the words as they came back in one array."""
        n = len(self.on_device)
        return got[:n], (None if self.dev_info is None else got[n:n + self.dev_info.numel()].reshape(self.dev_info.shape))

    def words_on_host(self):
        return read_back([self])[1][0]

    def file_bytes(self, i: int) -> bytes:
        if i in self.unstaged:
            return self.unstaged[i]
        return self.buffer[self.offsets[i]:self.offsets[i] + self.sizes[i]].cpu().numpy().tobytes()

    def finish(self, got_flags: np.ndarray, got_info: Optional[np.ndarray] = None) -> DecodedImages:
        n = len(self.sizes)
        images: List[Optional[Tensor]] = [None] * n
        flags = np.full(n, -1, dtype=np.int32)
        got = np.asarray(got_flags).tolist()
        for k, i in enumerate(self.on_device):  # too few flags: IndexError
            row, flag = self.rows[k], got[k]
            flags[i] = flag
            if flag == 0:
                images[i] = self.out[row[5]:row[5] + row[2] * row[6]].view(row[2], row[3], row[7])
        for i in range(n):
            if images[i] is None:  # never silent data: PIL's pixels, or PIL's error
                images[i] = torch.from_numpy(np.array(self.decoder._pil_decode(self.file_bytes(i), self.channels))).to(self.decoder.device)
        return self.decoder._result(images, flags, self.on_device, got_flags, got_info)


class PackedDecoder:
    """The decoder of one format. A subclass gives `_MODE` (channels -> PIL mode), `_header(data)` (what sizes an output, or
    None), `_pil_decode(data, channels)`, `_OPTIONS` (the names of its own keyword options, which go on to `_plan` and `_run`),
    `_heads_of(buffer, offsets, sizes)`, `_INFO` (the trailing shape of its info words, or None), `_plan(rows, **options)` (the
    descriptor as the library takes it, the scratch bytes, what `_run` needs besides), `_run(...)` (the launch: the library's status)
    and `_result(images, flags, on_device, got_flags, got_info)`."""

    _MODE: dict = {}
    _INFO: Optional[tuple] = None
    _OPTIONS: tuple = ()

    def __init__(self, device: Optional[Union[int, torch.device]] = None):
        self.device = cuda_device(device)
        self._lib = _lib.load()

    def _check_channels(self, channels: Optional[int]) -> None:
        if channels is not None and channels not in self._MODE:
            raise ValueError(f"channels must be None or one of {sorted(self._MODE)}, got {channels}")

    def decode(self, sources: Sequence[Source], channels: Optional[int] = None, **options) -> DecodedImages:
        """`sources`: paths or bytes. `channels`: None keeps each file's own; a key of `_MODE` converts as PIL's `convert` to that
        mode does. One synchronisation: the flags, and the format's info words beside them."""
        pending = self._launch(sources, channels, **options)
        return pending.finish(*pending.words_on_host())

    def _launch(self, sources: Sequence[Source], channels: Optional[int] = None, **options) -> PendingDecode:
        """`decode` without its synchronisation. Packs the files the device will read into one pinned buffer (a file the host cannot
        size goes to PIL as it is), then `_launch_packed`."""
        self._check_channels(channels)
        files = [bytes_of(s) for s in sources]
        heads = [self._header(f) for f in files]
        staged, table = pack([f if h is not None else b"" for f, h in zip(files, heads)], pinned=True)
        offsets, sizes = table.T.tolist()
        pending = self._launch_packed(staged, offsets, sizes, channels, heads=heads, **options)
        pending.unstaged = {i: f for i, (f, h) in enumerate(zip(files, heads)) if h is None}
        return pending

    def decode_packed(self, buffer: Tensor, offsets: Sequence[int], sizes: Sequence[int], channels: Optional[int] = None,
                      heads: Optional[Sequence] = None, **options) -> DecodedImages:
        """`decode` for files that already lie in one uint8 buffer, on the CPU (ideally pinned) or on the device: file i is
        buffer[offsets[i] : offsets[i] + sizes[i]], every offset a multiple of 16 and the buffer long enough to hold every file
        rounded up to 16 bytes (`align`). `heads`: `_header` of every file where the caller has read it already; a buffer is
        otherwise asked for them (`_heads_of`). One synchronisation, as in `decode`."""
        pending = self._launch_packed(buffer, offsets, sizes, channels, heads=heads, **options)
        return pending.finish(*pending.words_on_host())

    def _launch_packed(self, buffer, offsets, sizes, channels=None, heads=None, **options) -> PendingDecode:
        """The launches of `decode_packed` without its synchronisation: the caller reads the pending's `words()` back with whatever
        else it waits for (`read_back`) and hands them to `.finish`."""
        if set(options) - set(self._OPTIONS):
            raise TypeError(f"{type(self).__name__}: unexpected keyword arguments {sorted(set(options) - set(self._OPTIONS))}")
        self._check_channels(channels)
        offsets, sizes = check_packed(buffer, offsets, sizes, heads)
        if heads is None:
            heads = self._heads_of(buffer, offsets, sizes)
        heads = [None if h is None else tuple(int(v) for v in h) for h in heads]
        pending = PendingDecode(self, buffer, offsets, sizes, channels, heads)
        if pending.on_device:
            dev = self.device
            rows, out_at = descriptor_rows(offsets, sizes, heads, channels, pending.on_device)
            desc, scratch_bytes, plan = self._plan(rows, **options)
            if scratch_bytes == 0:
                raise _lib.Dad3dError(_lib.E_INVALID, f"{type(self).__name__}: the library's scratch_bytes call refused the batch")
            data = buffer.to(dev, non_blocking=True)  # one H2D transfer (none for a buffer on the device)
            desc_dev = torch.from_numpy(desc).pin_memory().to(dev, non_blocking=True)  # from pinned memory: the host does not wait
            out = torch.empty(out_at, dtype=torch.uint8, device=dev)
            pending.dev_flags = torch.empty(len(rows), dtype=torch.int32, device=dev)
            if self._INFO is not None:
                pending.dev_info = torch.empty((len(rows),) + self._INFO, dtype=torch.int32, device=dev)
            scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
            _lib.check(self._run(plan, data, desc_dev, len(rows), out, pending.dev_flags, pending.dev_info, scratch, device_index(dev),
                                 torch.cuda.current_stream(dev).cuda_stream, **options))
            pending.rows, pending.out, pending.data = rows, out, data
        return pending
