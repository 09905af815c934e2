"""`json.load` with the large arrays of numbers read on the MI355X (csrc/json_parse.hip): what `DADEvaluator` spends
99.9 % of its time in (dad_3dheads_benchmark/benchmark.py:177-180).

`load(path_or_bytes)` copies the document to the device in one transfer. The kernels index it (string state, bracket depth, number
tokens), the regular arrays of numbers of one or two levels with at least `min_count` values are validated there and converted to
float64 with the bits `json.loads` would give (json_parse_number.hpp: exact integer arithmetic), and every lifted span is replaced by
a one-key placeholder object in a small skeleton text that `json.loads` parses on the host. The device lifts only what it has fully
validated; whatever it is unsure of stays in the skeleton, so the tree can differ from `json.loads` in nothing but speed.

Between the kernels, the bracket list is matched (a stable sort by depth) and the arrays are chosen with torch list operations; these
run on lists of brackets and arrays, never on the bytes.
"""
from __future__ import annotations

import json
import os
import secrets
from typing import Any, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._packed_files import cuda_device

PLACEHOLDER_KEY = "__dad3d_device_array__"
_PLACEHOLDER_BYTES = PLACEHOLDER_KEY.encode("ascii")
MAX_BYTES = 2 ** 31 - 1


class DeviceArray:
    """One lifted array: `count` float64 values of `JsonDocument.values` from `offset`, of shape (n,) or (rows, n / rows)."""

    __slots__ = ("_doc", "offset", "count", "shape")

    @property
    def document(self) -> "JsonDocument":
        return self._doc

    @property
    def size(self) -> int:
        return self.count

    def __init__(self, doc: "JsonDocument", offset: int, count: int, rows: int):
        self._doc = doc
        self.offset = int(offset)
        self.count = int(count)
        self.shape = (self.count,) if rows == 0 else (int(rows), self.count // int(rows))

    def __len__(self) -> int:
        return self.shape[0]

    def tensor(self) -> Tensor:
        """float64 view of the document's values (no copy)."""
        return self._doc.values[self.offset:self.offset + self.count].view(self.shape)

    def float32(self) -> Tensor:
        """Cast on the device, round to nearest even: the bits of `np.asarray(list, dtype=np.float32)`."""
        return self.tensor().to(torch.float32)

    def tolist(self) -> list:
        """The list `json.loads` holds in this place: Python floats, and ints where the token had no fraction or exponent part."""
        values, is_int = self._doc._host()
        v = values[self.offset:self.offset + self.count]
        i = is_int[self.offset:self.offset + self.count]
        if not i.any():
            flat: Any = v
        elif i.all():
            flat = v.astype(np.int64)
        else:
            flat = np.empty(self.count, dtype=object)
            flat[:] = [int(x) if k else x for x, k in zip(v.tolist(), i.tolist())]
        return flat.reshape(self.shape).tolist()

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.tolist(), dtype=dtype)

    def __repr__(self) -> str:
        return f"DeviceArray(shape={self.shape}, offset={self.offset})"


class JsonDocument:
    """`.root`: the tree `json.loads` returns with `DeviceArray` handles in place of the lifted arrays; `.values` float64 and `.is_int`
    uint8 on the device, one entry per lifted number; `.records` int32 [n, 6] on the host: byte of `[`, byte behind `]`, first value
    index, count, rows (0: one level), first token index."""

    def __init__(self, values: Tensor, is_int: Tensor, records: np.ndarray):
        self.values = values
        self.is_int = is_int
        self.records = records
        self.arrays: List[DeviceArray] = [DeviceArray(self, r[2], r[3], r[4]) for r in records.tolist()]
        self.root: Any = None
        self._cpu: Optional[Tuple[np.ndarray, np.ndarray]] = None

    def _host(self) -> Tuple[np.ndarray, np.ndarray]:
        if self._cpu is None:
            self._cpu = (self.values.cpu().numpy(), self.is_int.cpu().numpy().astype(bool))
        return self._cpu

    def to_python(self) -> Any:
        """The plain tree: handles become lists, ints are restored."""
        def walk(x):
            if isinstance(x, DeviceArray):
                return x.tolist()
            if isinstance(x, dict):
                return {k: walk(v) for k, v in x.items()}
            if isinstance(x, list):
                return [walk(v) for v in x]
            return x
        return walk(self.root)


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _empty(dev: torch.device) -> Tuple[Tensor, Tensor, np.ndarray]:
    return (torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.uint8, device=dev),
            np.zeros((0, _lib.JSON_PARSE_RECORD_INTS), dtype=np.int32))


def lift(text: Tensor, min_count: int = 32, events: Optional[list] = None) -> Tuple[Tensor, Tensor, np.ndarray]:
    """The device part: `text` uint8 CUDA, 1 <= len < 2^31 -> (values float64, is_int uint8, records int32 [n, 6] on the host).
    `events`: a list that receives (entry name, start event, end event) around each of the four library calls, for the bench."""
    lib = _lib.load()
    dev = text.device
    assert text.is_cuda and text.dtype == torch.uint8 and text.ndim == 1 and text.is_contiguous()
    n = text.numel()
    assert 0 < n <= MAX_BYTES
    idx, st = dev.index or 0, _stream(dev)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731

    def call(name, *args):
        if events is None:
            return _lib.check(getattr(lib, name)(*args, idx, st))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(getattr(lib, name)(*args, idx, st))
        e1.record()
        events.append((name, e0, e1))

    scratch_bytes = lib.dad3d_json_parse_scratch_bytes(n)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    counts = i32(4)
    call("dad3d_json_parse_index", text.data_ptr(), n, scratch.data_ptr(), scratch_bytes, counts.data_ptr())
    n_tok, n_brk, _, _ = counts.tolist()  # the sync: the sizes of the lists
    if n_tok == 0 or n_brk < 2:
        return _empty(dev)
    tok_pos, tok_brk = i32(n_tok), i32(n_tok)
    brk_pos, brk_key, brk_nonnum, brk_tok = i32(n_brk), i32(n_brk), i32(n_brk), i32(n_brk)
    call("dad3d_json_parse_lists", text.data_ptr(), n, scratch.data_ptr(), scratch_bytes, tok_pos.data_ptr(), tok_brk.data_ptr(), n_tok,
         brk_pos.data_ptr(), brk_key.data_ptr(), brk_nonnum.data_ptr(), brk_tok.data_ptr(), n_brk)
    del scratch

    # match the brackets: in a stable order by depth key a `[` is followed by its `]` (no bracket of the same key lies between them)
    is_open = text[brk_pos.long()] == 0x5B
    order = torch.sort(brk_key, stable=True).indices
    s_open, s_key = is_open[order], brk_key[order]
    pair = s_open[:-1] & ~s_open[1:] & (s_key[:-1] == s_key[1:])
    arr_open, by_pos = torch.sort(order[:-1][pair])
    arr_close = order[1:][pair][by_pos]
    # numeric: no non-numeric byte inside. maximal: not inside an earlier numeric array (spans nest or are disjoint)
    numeric = brk_nonnum[arr_close] == brk_nonnum[arr_open]
    arr_open, arr_close = arr_open[numeric], arr_close[numeric]
    if arr_open.numel() == 0:
        return _empty(dev)
    closed_before = torch.cat([arr_close.new_full((1,), -1), torch.cummax(arr_close, 0).values[:-1]])
    count = brk_tok[arr_close] - brk_tok[arr_open]
    keep = (arr_open > closed_before) & (count >= max(int(min_count), 1))
    arr_open, arr_close, count = arr_open[keep].int().contiguous(), arr_close[keep].int().contiguous(), count[keep]
    n_arr = arr_open.numel()
    if n_arr == 0:
        return _empty(dev)
    rows = i32(n_arr)
    call("dad3d_json_parse_check_arrays", text.data_ptr(), n, tok_pos.data_ptr(), tok_brk.data_ptr(), n_tok, brk_pos.data_ptr(), brk_key.data_ptr(),
         brk_tok.data_ptr(), n_brk, arr_open.data_ptr(), arr_close.data_ptr(), rows.data_ptr(), n_arr)
    ok = rows >= 0
    arr_open, arr_close, count, rows = arr_open[ok].long(), arr_close[ok].long(), count[ok], rows[ok]
    if arr_open.numel() == 0:
        return _empty(dev)
    total = torch.cumsum(count, 0)
    records = torch.stack([brk_pos[arr_open], brk_pos[arr_close] + 1, (total - count).int(), count.int(), rows, brk_tok[arr_open]], 1).int().contiguous()
    host_records = records.cpu().numpy()
    n_values = int(host_records[-1, 2]) + int(host_records[-1, 3])
    values = torch.empty(n_values, dtype=torch.float64, device=dev)
    is_int = torch.empty(n_values, dtype=torch.uint8, device=dev)
    call("dad3d_json_parse_extract", text.data_ptr(), n, tok_pos.data_ptr(), n_tok, records.data_ptr(), records.shape[0], n_values, values.data_ptr(),
         is_int.data_ptr(), n_values)
    return values, is_int, host_records


def _read(source: Union[str, os.PathLike, bytes, bytearray, memoryview]) -> Tensor:
    """The document's bytes in a pinned host buffer."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        view = memoryview(source).cast("B")
        pinned = torch.empty(len(view), dtype=torch.uint8, pin_memory=len(view) > 0)
        pinned.numpy()[:] = np.frombuffer(view, dtype=np.uint8)
        return pinned
    size = os.path.getsize(source)
    pinned = torch.empty(size, dtype=torch.uint8, pin_memory=size > 0)
    with open(source, "rb") as f:
        got = f.readinto(memoryview(pinned.numpy())) if size else 0
    if got != size:
        raise OSError(f"{source}: read {got} of {size} bytes")
    return pinned


def _host_document(data: bytes, dev: torch.device) -> JsonDocument:
    doc = JsonDocument(*_empty(dev))
    doc.root = json.loads(data)
    return doc


def load(source: Union[str, os.PathLike, bytes, bytearray, memoryview], device: Optional[Union[int, torch.device]] = None,
         min_count: int = 32) -> JsonDocument:
    """`json.load` of a file (or of `bytes`) with every regular array of at least `min_count` numbers left on the device.

    Raises `json.JSONDecodeError` for a malformed document, as `json.loads` does. A document that holds the placeholder key, or is
    2 GiB or larger, is parsed on the host alone."""
    dev = cuda_device(device)
    pinned = _read(source)
    n = pinned.numel()
    data = pinned.numpy().tobytes() if n <= MAX_BYTES else None
    if n == 0 or n > MAX_BYTES or _PLACEHOLDER_BYTES in data:
        return _host_document(data if data is not None else pinned.numpy().tobytes(), dev)
    text = pinned.to(dev, non_blocking=True)  # one H2D transfer
    values, is_int, records = lift(text, min_count)
    doc = JsonDocument(values, is_int, records)
    if not len(records):
        doc.root = json.loads(data)
        return doc
    # the key ends in a nonce of this call: no spelling of it (escapes included) can be in the document
    key = PLACEHOLDER_KEY + secrets.token_hex(8)
    pieces, at = [], 0
    for i, r in enumerate(records.tolist()):
        pieces.append(data[at:r[0]])
        pieces.append(b'{"%s":%d}' % (key.encode("ascii"), i))
        at = r[1]
    pieces.append(data[at:])
    arrays = doc.arrays

    def hook(obj):
        if len(obj) == 1 and key in obj:
            return arrays[obj[key]]
        return obj

    try:
        doc.root = json.loads(b"".join(pieces), object_hook=hook)
    except json.JSONDecodeError:
        return _host_document(data, dev)  # raises with the position in the document itself
    return doc
