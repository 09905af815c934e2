"""On-disk formats downstream of the decode: the `.obj` mesh text and the FLAME-parameter JSON of the
reference's demo (`demo_utils.py:106-153`). Same bytes as `MeshSaver` / `JsonSaver` write; the batch variants format a
whole batch of decoded meshes with the constant face block rendered once.

The vertex block of a float32 CUDA batch is formatted on the GPU (`ObjFormatter`, csrc/obj_text.hip: the same bytes from 64-bit
integer arithmetic); a mesh that holds a value outside the kernel's domain (NaN, inf, |x| >= 2^37) is flagged
there and formatted by `_vertex_block` here. The face block (a constant) and `MeshSaver.__call__` for one host mesh stay on the
host.

JSON of a float32 CUDA batch is formatted on the GPU too (`JsonFormatter`, csrc/json_text.hip): a `JsonTemplate`
holds the literal bytes of one item's layout, the numbers between them are `float.__repr__` of the value widened to double --
the shortest round-trip form `json.dump` prints -- from 128-bit integer products. `flame_params_json_batch` /
`save_flame_params_batch` write the bytes of `JsonSaver` that way; an item that holds NaN or an infinity is flagged on the device
and formatted here (`_json_item_host`). `JsonSaver`, `get_flame_params` and `flame_params_batch` are the host path, unchanged.

Images (`ImageSaver` of the demo, demo_utils.py:122-127) are written as PNG: a uint8 CUDA batch is filtered, deflated and framed on
the GPU (`PngEncoder`, csrc/png_encode.hip; `png_batch`, `save_png_batch`), a host image by PIL (`ImageSaver`).
Where a lossy file is wanted -- photographs with overlays, renders over a background -- `JpegEncoder` (csrc/jpeg_encode.hip,
DESIGN.md 4.20; `jpeg_batch`, `save_jpeg_batch`) writes baseline JPEG on the GPU with the bytes PIL writes for the same options.
Both are `_ImageEncoder`: one argument check, one encode body, one cache, one device-path predicate and one write loop.
"""
from __future__ import annotations

import io
import json
import os
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .flame import _SLICE_ORDER, FLAME_CONSTS, FlameParams


def get_mesh(predictions: Dict[str, torch.Tensor], faces: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """demo_utils.py:106-109: vertices [N,3] and faces as FLOATS shifted to 1-based indices (`+ 1.`)."""
    return predictions["3d_vertices"].detach().cpu().numpy(), np.asarray(faces) + 1.0


def get_uv_texture(predictions: Dict[str, torch.Tensor], image: np.ndarray, creator) -> np.ndarray:
    """demo_utils.py:97-100 with the creator passed in (the reference builds a `UVTextureCreator()` per call, which loads its
    atlas and model files): uint8 [S,S,3]; zeroes translation z in `predictions["3dmm_params"]` like the reference."""
    return creator(image, predictions)


def get_flame_params(predictions: Dict[str, torch.Tensor], constants: Dict[str, int] = FLAME_CONSTS) -> Dict[str, List[float]]:
    """demo_utils.py:112-116: {"shape": [...], "expression": [...], ...} of the first row."""
    fp = FlameParams.from_3dmm(predictions["3dmm_params"].detach().cpu(), constants)
    return {k: v[0].tolist() for k, v in vars(fp).items()}


def _vertex_block(vertices: np.ndarray) -> str:
    buf = io.StringIO()
    np.savetxt(buf, np.asarray(vertices).reshape(-1, 3), fmt="v %.8f %.8f %.8f")  # '%'-formatting row by row, '\n' ends
    return buf.getvalue()


def _face_block(faces_1based: np.ndarray) -> str:
    buf = io.StringIO()
    np.savetxt(buf, np.asarray(faces_1based).reshape(-1, 3), fmt="f %d %d %d")
    return buf.getvalue()


def obj_text(vertices: np.ndarray, faces_1based: np.ndarray) -> str:
    """The text `MeshSaver.__call__` writes (demo_utils.py:130-144): `v %.8f %.8f %.8f` lines, then `f %d %d %d`."""
    return _vertex_block(vertices) + _face_block(faces_1based)


class MeshSaver:
    def __init__(self) -> None:
        self.extension = ".obj"

    def __call__(self, mesh: Tuple[np.ndarray, np.ndarray], output_path: str) -> None:
        vertices, faces = mesh
        with open(output_path, "w") as f:
            f.write(obj_text(vertices, faces))


class JsonSaver:
    def __init__(self) -> None:
        self.extension = ".json"

    def __call__(self, flame_params: Dict[str, List[float]], output_path: str) -> None:
        with open(output_path, "w") as out:
            json.dump(flame_params, out)


def _check_batch(name: str, t: Any, dtype: torch.dtype, shape: Tuple[int, ...], device: torch.device) -> None:
    """ValueError unless `t` is a contiguous `dtype` tensor [B, *shape] on `device`."""
    if (not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or not t.is_contiguous() or t.ndim != len(shape) + 1
            or tuple(t.shape[1:]) != tuple(shape)):
        raise ValueError(f"{name}: expected a contiguous {str(dtype)[6:]} tensor [B,{','.join(str(v) for v in shape)}] on {device}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', 'the host')}"
                         + ("" if not isinstance(t, torch.Tensor) or t.is_contiguous() else " (not contiguous)"))


def _write_blocks(blocks: Sequence[Any], paths: Sequence[str], tail: bytes = b"") -> None:
    """One file per block of bytes, each with `tail` behind it."""
    for block, path in zip(blocks, paths):
        with open(path, "wb") as f:
            f.write(block)
            if tail:
                f.write(tail)


class _DeviceText:
    """Text of `batch` items in a formatter's HBM buffer. Item b's bytes are `text[b, :lengths[b]]` (byte offset `b * stride` of
    the buffer); `flags[b] != 0` marks an item the kernel left to the host (`_host_item`). The buffers belong to the formatter:
    they hold this batch until its next `format`."""

    def __init__(self, formatter: "_TextBuffers", batch: int):
        self.formatter, self.batch = formatter, batch
        self.text, self.stride = formatter._text[:batch], formatter.stride
        self.lengths, self.flags = formatter._lengths[:batch], formatter._flags[:batch]
        self.offsets = [b * self.stride for b in range(batch)]
        self._copy: Optional[Tuple[np.ndarray, np.ndarray, int, torch.cuda.Event]] = None

    def _host_item(self, b: int) -> bytes:
        raise NotImplementedError

    def begin_host_copy(self) -> None:
        """Waits for the lengths and flags (one small copy), then enqueues the copy of the text that exists -- `batch` rows of the
        longest item's length, not of the worst-case stride -- into the formatter's pinned buffer, without waiting for it."""
        if self._copy is not None:
            return
        f, b = self.formatter, self.batch
        f._meta_host.copy_(f._meta, non_blocking=True)
        torch.cuda.current_stream(f.torch_device).synchronize()
        meta = f._meta_host.numpy()
        lengths = meta[: 8 * b].view(np.int64).copy()
        flags = meta[8 * f.capacity : 8 * f.capacity + 4 * b].view(np.int32).copy()
        width = int(lengths.max()) if b else 0
        if width:
            packed = self.text[:, :width].contiguous()  # rows at the stride -> rows at `width`: one dense copy out
            f._host[: b * width].copy_(packed.view(-1), non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(f.torch_device))
        self._copy = (lengths, flags, width, done)

    def to_host(self) -> List[Any]:
        """The text of every item as bytes on the host: a `memoryview` into the formatter's pinned buffer (valid until its next
        `to_host`), or `bytes` from the host formatter for a flagged item."""
        self.begin_host_copy()
        lengths, flags, width, done = self._copy
        done.synchronize()
        host = memoryview(self.formatter._host.numpy())
        out: List[Any] = []
        for b in range(self.batch):
            if flags[b]:
                out.append(self._host_item(b))
            else:
                out.append(host[b * width : b * width + int(lengths[b])])
        return out


class _TextBuffers:
    """The buffers of a device text formatter: `capacity` rows of `stride` bytes of text, lengths and flags, the kernels' scratch
    and the pinned host side of the copy. A subclass sets `stride` and gives `_scratch_bytes_for(batch)`."""

    def __init__(self, device: Optional[int] = None):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.torch_device = torch.device("cuda", self.device)
        self.capacity = 0

    def reserve(self, batch: int) -> None:
        batch = max(int(batch), 1)
        if batch > self.capacity:
            self._reserve_buffers(batch, self._scratch_bytes_for(batch))

    def _reserve_buffers(self, batch: int, scratch_bytes: int) -> None:
        dev = self.torch_device
        self.capacity = batch
        self._text = torch.empty((batch, max(self.stride, 16)), dtype=torch.uint8, device=dev)
        self._meta = torch.zeros(12 * batch, dtype=torch.uint8, device=dev)  # lengths int64 [batch] | flags int32 [batch]
        self._lengths, self._flags = self._meta[: 8 * batch].view(torch.int64), self._meta[8 * batch :].view(torch.int32)
        self._scratch_bytes = int(scratch_bytes)
        self._scratch = torch.empty(max(self._scratch_bytes, 8), dtype=torch.uint8, device=dev)
        self._meta_host = torch.empty(12 * batch, dtype=torch.uint8).pin_memory()
        self._host = torch.empty(batch * max(self.stride, 16), dtype=torch.uint8).pin_memory()


class ObjText(_DeviceText):
    """What `ObjFormatter.format` returns: the vertex text of `batch` meshes in HBM. Mesh b's bytes are
    `text[b, :lengths[b]]` (byte offset `b * stride` of the buffer); `flags[b] != 0` marks a mesh the kernel left to the host.
    The buffers belong to the formatter: they hold this batch until its next `format`."""

    def __init__(self, formatter: "ObjFormatter", vertices: torch.Tensor, batch: int):
        super().__init__(formatter, batch)
        self.vertices = vertices

    def _host_item(self, b: int) -> bytes:
        return _vertex_block(self.vertices[b].detach().cpu().numpy()).encode("ascii")


class ObjFormatter(_TextBuffers):
    """The `v %.8f %.8f %.8f` lines of a batch of meshes, formatted on the GPU (`dad3d_obj_format_vertices`).

    `reserve(batch)` allocates the device text buffer (`batch` rows of the worst case, 71 bytes per line), lengths, flags,
    scratch and one pinned host buffer; `format(vertices)` launches on the current stream with no allocation and no sync once
    the batch fits (capturable in a graph); `ObjText.to_host()` brings the bytes over. `faces` (0-based, as `save_obj_batch`
    takes them) gives `face_text`, the constant block behind every mesh's vertices."""

    def __init__(self, n_verts: int, faces: Optional[np.ndarray] = None, device: Optional[int] = None):
        super().__init__(device)
        self.n_verts = int(n_verts)
        self.stride = (self.n_verts * _lib.OBJ_MAX_LINE_BYTES + 15) // 16 * 16
        self.face_text = b"" if faces is None else _face_block(np.asarray(faces) + 1.0).encode("ascii")

    def _scratch_bytes_for(self, batch: int) -> int:
        return self._lib.dad3d_obj_format_scratch_bytes(batch, self.n_verts)

    def format(self, vertices: torch.Tensor) -> ObjText:
        _check_batch("vertices", vertices, torch.float32, (self.n_verts, 3), self.torch_device)
        b = vertices.shape[0]
        self.reserve(b)
        stream = torch.cuda.current_stream(self.torch_device).cuda_stream
        _lib.check(self._lib.dad3d_obj_format_vertices(vertices.data_ptr(), b, self.n_verts, self._text.data_ptr(), self._text.stride(0),
                                                       self._lengths.data_ptr(), self._flags.data_ptr(), self._scratch.data_ptr(),
                                                       self._scratch.numel(), self.device, stream))
        return ObjText(self, vertices, b)


_formatters: Dict[Tuple[int, int], ObjFormatter] = {}


def _formatter_for(vertices: torch.Tensor) -> ObjFormatter:
    key = (vertices.device.index, int(vertices.shape[1]))
    f = _formatters.get(key)
    if f is None:
        f = _formatters[key] = ObjFormatter(key[1], device=key[0])
    return f


def _on_device_path(vertices: Any) -> bool:
    return (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.ndim == 3
            and vertices.shape[-1] == 3 and vertices.is_contiguous())


def obj_text_batch(vertices: torch.Tensor, faces_1based: np.ndarray) -> List[bytes]:
    """The batched sibling of `obj_text`: `vertices [B,N,3]` -> the bytes of every mesh's `.obj` (vertex lines, then the face
    block of `faces_1based`, formatted once). A contiguous float32 CUDA tensor is formatted on the GPU; anything else by
    `obj_text`'s host path."""
    face_text = _face_block(faces_1based).encode("ascii")
    if _on_device_path(vertices):
        return [bytes(v) + face_text for v in _formatter_for(vertices).format(vertices.detach()).to_host()]
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    assert v.ndim == 3
    return [_vertex_block(row).encode("ascii") + face_text for row in v]


def _write_obj_files(blocks: Sequence[Any], face_text: bytes, paths: Sequence[str]) -> None:
    _write_blocks(blocks, paths, face_text)


def save_obj_batch(vertices: torch.Tensor, faces: np.ndarray, paths: Sequence[str], formatter: str = "auto") -> None:
    """`vertices [B,N,3]` (any device) -> one `.obj` per row; the face block is the same text for every mesh and is formatted
    once. A contiguous float32 CUDA tensor has its vertex lines formatted on the GPU (`ObjFormatter`; a flagged mesh is
    formatted here, mesh by mesh) and only text crosses to the host. A CPU tensor, another dtype, a non-contiguous tensor or
    `formatter="host"` takes the host path: one device-to-host copy of the floats, `np.savetxt` per mesh. Same bytes either way."""
    if formatter not in ("auto", "host"):
        raise ValueError(f"formatter: expected 'auto' or 'host', got {formatter!r}")
    assert vertices.ndim == 3 and vertices.shape[0] == len(paths)
    if formatter == "auto" and _on_device_path(vertices):
        face_text = _face_block(np.asarray(faces) + 1.0).encode("ascii")
        _write_obj_files(_formatter_for(vertices).format(vertices.detach()).to_host(), face_text, paths)
        return
    v = vertices.detach().cpu().numpy()
    face_text = _face_block(np.asarray(faces) + 1.0)
    for row, path in zip(v, paths):
        with open(path, "w") as f:
            f.write(_vertex_block(row))
            f.write(face_text)


def save_obj_from_params(head_mesh, params: torch.Tensor, paths: Sequence[str], faces: Optional[np.ndarray] = None,
                         batch_size: int = 64) -> None:
    """`params [M,413]` -> one `.obj` per row: decode (`head_mesh.vertices_3d`), format and write in batches of `batch_size`,
    the files `save_obj_batch(head_mesh.vertices_3d(params), faces, paths)` writes; the decoded floats never visit the host.
    `faces` defaults to the packaged FLAME topology. With more than one batch the decode, format and text copy of batch i + 1
    run on a side stream while the host writes the files of batch i (two formatters: two device and two pinned buffers)."""
    from .synthetic import load_static

    flame = head_mesh.flame
    dev = flame.torch_device
    assert params.ndim == 2 and params.shape[0] == len(paths)
    staged = params.detach().to(dev, torch.float32).contiguous()
    face_text = _face_block(np.asarray(load_static()["faces"] if faces is None else faces) + 1.0).encode("ascii")
    starts = list(range(0, len(paths), max(1, int(batch_size))))
    pair = [ObjFormatter(int(flame.n_verts), device=dev.index) for _ in range(min(2, len(starts)))]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))

    def launch(i: int) -> ObjText:
        with torch.cuda.stream(side), torch.no_grad():
            rows = staged[starts[i] : starts[i] + batch_size]
            text = pair[i % 2].format(flame.decode(rows, verts3d=True)["verts3d"])
            text.begin_host_copy()
        return text

    pending = launch(0) if starts else None
    for i in range(len(starts)):
        with torch.cuda.stream(side):
            blocks = pending.to_host()
        # batch i + 1 goes to the other formatter: its kernels and copy run while the files below are written
        pending = launch(i + 1) if i + 1 < len(starts) else None
        _write_obj_files(blocks, face_text, paths[starts[i] : starts[i] + batch_size])
    torch.cuda.current_stream(dev).wait_stream(side)


_SLOT = object()  # a number's place in the token stream of a template


def _structure_tokens(spec: Any) -> Iterable[Any]:
    if isinstance(spec, dict):
        yield "{"
        for i, (key, value) in enumerate(spec.items()):
            yield (", " if i else "") + json.dumps(str(key)) + ": "
            yield from _structure_tokens(value)
        yield "}"
    elif isinstance(spec, list):
        yield "["
        for i, value in enumerate(spec):
            if i:
                yield ", "
            yield from _structure_tokens(value)
        yield "]"
    elif isinstance(spec, tuple):  # a shape: () is one bare number
        if not spec:
            yield _SLOT
            return
        yield "["
        for i in range(int(spec[0])):
            if i:
                yield ", "
            yield from _structure_tokens(tuple(spec[1:]))
        yield "]"
    elif isinstance(spec, (int, np.integer)) and not isinstance(spec, bool) and spec >= 0:
        yield from _structure_tokens((int(spec),))  # a flat list of that many numbers
    else:
        raise ValueError(f"JsonTemplate: a leaf is a slot count or a shape (tuple), got {spec!r}")


class JsonTemplate:
    """The layout of one JSON item around its `n_slots` numbers: `literals[i]` is the text in front of number i, `literals[n_slots]`
    the suffix that closes the item. No literal may be longer than `_lib.JSON_MAX_LITERAL_BYTES` (ValueError)."""

    def __init__(self, literals: Sequence[bytes]):
        self.literals = [bytes(x) for x in literals]
        if not self.literals:
            raise ValueError("JsonTemplate: needs at least the suffix")
        self.n_slots = len(self.literals) - 1
        for i, lit in enumerate(self.literals):
            if len(lit) > _lib.JSON_MAX_LITERAL_BYTES:
                raise ValueError(f"JsonTemplate: literal {i} ({lit[:24]!r}...) is {len(lit)} bytes long, the formatter takes "
                                 f"{_lib.JSON_MAX_LITERAL_BYTES}")
        self.offsets = np.zeros(self.n_slots + 2, dtype=np.int32)
        np.cumsum([len(x) for x in self.literals], out=self.offsets[1:])
        self.literal_bytes = b"".join(self.literals)
        self.worst_case = len(self.literal_bytes) + self.n_slots * _lib.JSON_MAX_NUMBER_BYTES
        self.stride = max((self.worst_case + 15) // 16 * 16, 16)

    @classmethod
    def from_structure(cls, spec: Any) -> "JsonTemplate":
        """`spec`: nested dicts and lists as `json.dumps` renders them (separators `", "` and `": "`, keys through
        `json.dumps(str(k))`), with leaves that say where the numbers go: an int n is a flat list of n numbers (0: `[]`), a tuple
        is the shape of nested lists of numbers (`(68, 2)`: 68 pairs; `()`: one bare number)."""
        literals, cur = [], []
        for token in _structure_tokens(spec):
            if token is _SLOT:
                literals.append("".join(cur).encode("ascii"))
                cur = []
            else:
                cur.append(token)
        literals.append("".join(cur).encode("ascii"))
        return cls(literals)

    def render(self, numbers: Sequence[Any]) -> bytes:
        """The item with `numbers[i]` (bytes or str) in slot i."""
        assert len(numbers) == self.n_slots
        parts: List[bytes] = []
        for lit, num in zip(self.literals, numbers):
            parts.append(lit)
            parts.append(num if isinstance(num, bytes) else str(num).encode("ascii"))
        parts.append(self.literals[-1])
        return b"".join(parts)

    def device_image(self, device: torch.device) -> torch.Tensor:
        """What `dad3d_json_format_values` reads on the device: the int32 offsets, then the literal bytes."""
        image = np.frombuffer(self.offsets.tobytes() + self.literal_bytes, dtype=np.uint8).copy()
        return torch.from_numpy(image).to(device)


def _json_item_host(template: JsonTemplate, row: Any) -> bytes:
    """One item on the host, the numbers as `json.dumps` prints a float: `float.__repr__`, `NaN`, `Infinity`, `-Infinity`."""
    values = (row.detach().cpu() if isinstance(row, torch.Tensor) else torch.as_tensor(np.asarray(row))).to(torch.float64).reshape(-1)
    return template.render([json.dumps(v) for v in values.tolist()])


class JsonText(_DeviceText):
    """What `JsonFormatter.format` returns: the JSON text of `batch` items in HBM, the contract of `ObjText`. A flagged item
    (NaN, an infinity, or a flag the caller ORed in) is formatted on the host: by `host_item(b)` when the caller gave one, else
    from the float32 values by `_json_item_host`."""

    def __init__(self, formatter: "JsonFormatter", values: torch.Tensor, batch: int, host_item=None):
        super().__init__(formatter, batch)
        self.values, self.host_item = values, host_item

    def _host_item(self, b: int) -> bytes:
        if self.host_item is not None:
            return self.host_item(b)
        return _json_item_host(self.formatter.template, self.values[b])


class JsonFormatter(_TextBuffers):
    """The JSON text of a batch of items of one layout, formatted on the GPU (`dad3d_json_format_values`).

    `reserve(batch)` allocates the device text buffer (`batch` rows of the template's worst case: its literal bytes + 23 per
    number), lengths, flags, scratch, a float32 staging buffer `[batch, n_slots]` (`staging(batch)`: for callers that gather
    their fields on the device) and one pinned host buffer; `format(values)` launches on the current stream with no allocation
    and no sync once the batch fits (capturable in a graph); `JsonText.to_host()` brings the bytes over."""

    def __init__(self, template: JsonTemplate, device: Optional[int] = None):
        super().__init__(device)
        if template.n_slots < 1:
            raise ValueError("JsonFormatter: a template without numbers is a constant: template.render([])")
        self.template, self.n_slots, self.stride = template, template.n_slots, template.stride
        self._image = template.device_image(self.torch_device)
        self._offsets = np.ascontiguousarray(template.offsets)

    def _scratch_bytes_for(self, batch: int) -> int:
        return self._lib.dad3d_json_format_scratch_bytes(batch, self.n_slots)

    def _reserve_buffers(self, batch: int, scratch_bytes: int) -> None:
        super()._reserve_buffers(batch, scratch_bytes)
        self._staging = torch.zeros((batch, self.n_slots), dtype=torch.float32, device=self.torch_device)

    def staging(self, batch: int) -> torch.Tensor:
        self.reserve(batch)
        return self._staging[:batch]

    def format(self, values: torch.Tensor, host_item=None, extra_flags: Optional[torch.Tensor] = None) -> JsonText:
        """`values [B,n_slots]` -> `JsonText`. `extra_flags` (int32 [B] on the device) is ORed into the items' flags behind the
        kernels: a non-zero entry sends that item to `host_item(b)`."""
        _check_batch("values", values, torch.float32, (self.n_slots,), self.torch_device)
        b = values.shape[0]
        self.reserve(b)
        if b:
            stream = torch.cuda.current_stream(self.torch_device).cuda_stream
            _lib.check(self._lib.dad3d_json_format_values(values.data_ptr(), b, self.n_slots, self._image.data_ptr(), self._offsets.ctypes.data,
                                                          self._text.data_ptr(), self._text.stride(0), self._lengths.data_ptr(),
                                                          self._flags.data_ptr(), self._scratch.data_ptr(), self._scratch.numel(),
                                                          self.device, stream))
            if extra_flags is not None:
                self._flags[:b].bitwise_or_(extra_flags)
        return JsonText(self, values, b, host_item)


def _flame_params_layout(constants: Dict[str, int]) -> Tuple[Dict[str, int], List[int]]:
    """({key: count} in the key order of `get_flame_params`, the params column of every number in that order)."""
    first, cur = {}, 0
    for key in _SLICE_ORDER:
        first[key] = cur
        cur += int(constants[key])
    keys = list(vars(FlameParams.from_3dmm(torch.zeros((1, cur)), constants)))
    return {k: int(constants[k]) for k in keys}, [first[k] + i for k in keys for i in range(int(constants[k]))]


_json_formatters: Dict[Tuple[int, Tuple[Tuple[str, int], ...]], Tuple[JsonFormatter, torch.Tensor]] = {}


def _params_formatter_for(params: torch.Tensor, constants: Dict[str, int]) -> Tuple[JsonFormatter, torch.Tensor]:
    key = (params.device.index, tuple((k, int(v)) for k, v in constants.items()))
    hit = _json_formatters.get(key)
    if hit is None:
        spec, columns = _flame_params_layout(constants)
        fmt = JsonFormatter(JsonTemplate.from_structure(spec), device=key[0])
        hit = _json_formatters[key] = (fmt, torch.tensor(columns, dtype=torch.int64, device=params.device))
    return hit


def _params_on_device_path(params: Any, constants: Dict[str, int]) -> bool:
    return (isinstance(params, torch.Tensor) and params.is_cuda and params.dtype == torch.float32 and params.ndim == 2
            and params.is_contiguous() and params.shape[1] == sum(int(constants[k]) for k in _SLICE_ORDER) and params.shape[1] > 0)


def _format_flame_params(params: torch.Tensor, constants: Dict[str, int]) -> JsonText:
    fmt, columns = _params_formatter_for(params, constants)
    staged = fmt.staging(params.shape[0])
    torch.index_select(params.detach(), 1, columns, out=staged)  # the key order of the file is not the column order
    return fmt.format(staged)


def flame_params_json_batch(params: torch.Tensor, constants: Dict[str, int] = FLAME_CONSTS) -> List[bytes]:
    """`params [B,413]` -> the bytes `JsonSaver` writes for every row: row i is
    `json.dumps(get_flame_params({"3dmm_params": params[i:i+1]}, constants)).encode()`. A contiguous float32 CUDA tensor is
    formatted on the GPU; anything else by `json.dumps`."""
    if _params_on_device_path(params, constants):
        return [bytes(x) for x in _format_flame_params(params, constants).to_host()]
    return [json.dumps(d).encode("ascii") for d in flame_params_batch(params, constants)]


def save_flame_params_batch(params: torch.Tensor, paths: Sequence[str], formatter: str = "auto") -> None:
    """`params [B,413]` -> one flame_params `.json` per row, the files `JsonSaver()(get_flame_params(...), path)` writes. A
    contiguous float32 CUDA tensor is formatted on the GPU and only text crosses to the host; a CPU tensor, another dtype, a
    non-contiguous tensor or `formatter="host"` goes through `JsonSaver`. Same bytes either way."""
    if formatter not in ("auto", "host"):
        raise ValueError(f"formatter: expected 'auto' or 'host', got {formatter!r}")
    assert params.ndim == 2 and params.shape[0] == len(paths)
    if formatter == "auto" and _params_on_device_path(params, FLAME_CONSTS):
        _write_blocks(_format_flame_params(params, FLAME_CONSTS).to_host(), paths)
        return
    saver = JsonSaver()
    for row, path in zip(flame_params_batch(params), paths):
        saver(row, path)


def flame_params_batch(params: torch.Tensor, constants: Dict[str, int] = FLAME_CONSTS) -> List[Dict[str, List[float]]]:
    """`params [B,413]` -> the per-image dictionaries `get_flame_params` produces."""
    fp = FlameParams.from_3dmm(params.detach().cpu(), constants)
    fields = {k: v.tolist() for k, v in vars(fp).items()}
    return [{k: rows[i] for k, rows in fields.items()} for i in range(params.shape[0])]


def _png_host(image: np.ndarray) -> bytes:
    """One image on the host with PIL: uint8 [H,W,C], C = 1..4, stored in the order it is given."""
    from PIL import Image

    arr = np.ascontiguousarray(image)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if arr.dtype != np.uint8 or arr.ndim != 3 or not 1 <= arr.shape[2] <= 4:
        raise ValueError(f"image: expected uint8 [H,W,C] with C in 1..4, got {arr.dtype} {arr.shape}")
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(buf, format="PNG")  # L / LA / RGB / RGBA from the shape
    return buf.getvalue()


class ImageSaver:
    """demo_utils.py:122-127 without cv2: the reference swaps the channels for `cv2.imwrite`, which swaps them back when it writes,
    so the file holds the array's own order. One host image, encoded on the host (as `MeshSaver` stays on the host)."""

    def __init__(self) -> None:
        self.extension = ".png"

    def __call__(self, image: np.ndarray, output_path: str) -> None:
        with open(output_path, "wb") as f:
            f.write(_png_host(np.asarray(image)))


class _ImageData(_DeviceText):
    """What an image encoder's `encode` returns: the files of `batch` images in HBM, the contract of `ObjText`. A flagged item (the
    encoder's own consistency check, or a flag the caller ORed in) is encoded on the host with PIL, with the encoder's options."""

    def __init__(self, encoder: "_ImageEncoder", images: torch.Tensor, batch: int):
        super().__init__(encoder, batch)
        self.images = images

    def _host_item(self, b: int) -> bytes:
        return self.formatter._host_encode(self.images[b].detach().cpu().numpy(), **self.formatter.options)


PngData = JpegData = _ImageData


class _ImageEncoder(_TextBuffers):
    """A batch of uint8 images `[B,H,W,C]` as files made on the GPU. `reserve(batch)` allocates the device file buffer (`batch` rows
    of the format's worst case), lengths, flags, scratch and one pinned host buffer; `encode(images)` launches on the current stream
    with no allocation and no sync once the batch fits (capturable in a graph); `to_host()` of what it returns brings the files
    over. A format gives `_CHANNELS` (the channel counts it takes), `_LIMITS` (for the error text), `options` (what its host
    encoder takes besides the image), `_key_options`, `_max_bytes`, `_scratch_bytes_for`, `_launch` and `_host_encode`."""

    options: Dict[str, Any] = {}

    def __init__(self, height: int, width: int, channels: int, device: Optional[int] = None):
        super().__init__(device)
        self.height, self.width, self.channels = int(height), int(width), int(channels)
        worst = self._max_bytes()
        if worst == 0:
            raise ValueError(f"{type(self).__name__}: cannot encode images of {self.height} x {self.width} x {self.channels} ({self._LIMITS})")
        self.stride = (worst + 15) // 16 * 16

    @staticmethod
    def _key_options(channels: int, height: int, width: int) -> tuple:
        """The constructor's arguments behind `channels`, as the options of a `*_batch` call give them."""
        return ()

    def encode(self, images: torch.Tensor, extra_flags: Optional[torch.Tensor] = None) -> _ImageData:
        """`images [B,H,W,C]` -> the files. `extra_flags` (int32 [B] on the device) is ORed into the items' flags behind the
        kernels: a non-zero entry sends that item to the host encoder."""
        _check_batch("images", images, torch.uint8, (self.height, self.width, self.channels), self.torch_device)
        b = images.shape[0]
        self.reserve(b)
        if b:
            _lib.check(self._launch(images, b, torch.cuda.current_stream(self.torch_device).cuda_stream))
            if extra_flags is not None:
                self._flags[:b].bitwise_or_(extra_flags)
        return _ImageData(self, images, b)


class PngEncoder(_ImageEncoder):
    """`_ImageEncoder` for PNG, C = 1..4 (`dad3d_png_encode`, csrc/png_encode.hip, DESIGN.md 4.15, three kernels): row filters,
    deflate per segment of `_lib.PNG_SEGMENT_BYTES` with Huffman tables built on the device, CRC-32 and Adler-32. Lossless; the
    bytes are this encoder's own."""

    _CHANNELS = (1, 2, 3, 4)
    _LIMITS = "1..4 channels, a filtered stream below 2^31 bytes"

    def _max_bytes(self) -> int:
        return self._lib.dad3d_png_max_bytes(self.height, self.width, self.channels)

    def _scratch_bytes_for(self, batch: int) -> int:
        return self._lib.dad3d_png_scratch_bytes(batch, self.height, self.width, self.channels)

    def _launch(self, images: torch.Tensor, b: int, stream: int) -> int:
        return self._lib.dad3d_png_encode(images.data_ptr(), b, self.height, self.width, self.channels, self._text.data_ptr(),
                                          self._text.stride(0), self._lengths.data_ptr(), self._flags.data_ptr(), self._scratch.data_ptr(),
                                          self._scratch.numel(), self.device, stream)

    @staticmethod
    def _host_encode(image: np.ndarray, **options: Any) -> bytes:
        return _png_host(image, **options)


_encoders: Dict[tuple, _ImageEncoder] = {}


def _encoder_for(cls, images: torch.Tensor, **options: Any) -> _ImageEncoder:
    """One encoder of the format `cls` per (device, h, w, c, *options)."""
    h, w, c = (int(v) for v in images.shape[1:])
    key = (cls, images.device.index, h, w, c) + cls._key_options(c, h, w, **options)
    enc = _encoders.get(key)
    if enc is None:
        enc = _encoders[key] = cls(*key[2:], device=key[1])
    return enc


def _image_on_device_path(images: Any, channels: Sequence[int]) -> bool:
    return (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.uint8 and images.ndim == 4
            and images.shape[3] in channels and images.shape[1] >= 1 and images.shape[2] >= 1 and images.is_contiguous())


def _image_files(cls, images: Any, encoder: str, **options: Any) -> Sequence[Any]:
    """One file per image in the format of `cls`: from the GPU for a contiguous uint8 CUDA batch (unless `encoder="host"`), else
    from the format's host encoder, image by image."""
    if encoder == "auto" and _image_on_device_path(images, cls._CHANNELS):
        return _encoder_for(cls, images, **options).encode(images.detach()).to_host()
    arr = images.detach().cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    return [cls._host_encode(a, **options) for a in arr]


def _save_image_files(cls, images: Any, paths: Sequence[str], encoder: str, **options: Any) -> None:
    if encoder not in ("auto", "host"):
        raise ValueError(f"encoder: expected 'auto' or 'host', got {encoder!r}")
    assert len(images) == len(paths)
    _write_blocks(_image_files(cls, images, encoder, **options), paths)


def png_batch(images: Any) -> List[bytes]:
    """`images [B,H,W,C]` uint8 -> the bytes of one PNG file per image. A contiguous uint8 CUDA tensor is encoded on the GPU;
    anything else (a numpy array, a CPU tensor) by PIL on the host. The files differ in bytes and decode to the same pixels."""
    return [bytes(x) for x in _image_files(PngEncoder, images, "auto")]


def save_png_batch(images: Any, paths: Sequence[str], encoder: str = "auto") -> None:
    """`images [B,H,W,C]` uint8 -> one `.png` per image. A contiguous uint8 CUDA tensor is encoded on the GPU (`PngEncoder`; a
    flagged image is encoded here) and only the files cross to the host; a numpy array, a CPU tensor, a non-contiguous tensor or
    `encoder="host"` takes the host path: one copy of the pixels, PIL per image."""
    _save_image_files(PngEncoder, images, paths, encoder)


def _jpeg_options(channels: int, height: int, width: int, quality: int = 75, subsampling: Optional[int] = None,
                  restart_marker_rows: int = 0) -> Tuple[int, int, int, int]:
    """(quality, subsampling, restart_marker_rows, restart interval in MCUs) as libjpeg takes them: `None` is PIL's default for the
    mode (4:2:0 for RGB); grey has no subsampling; the interval is rows x MCUs per row, and a product above 65535, which libjpeg
    would clamp, is refused."""
    quality, rows = int(quality), int(restart_marker_rows)
    subsampling = 0 if channels == 1 else 2 if subsampling is None else int(subsampling)
    if channels not in (1, 3):
        raise ValueError(f"JPEG: {channels} channels (1 grey, 3 RGB)")
    if not 1 <= quality <= 100:
        raise ValueError(f"JPEG: quality {quality} outside 1 .. 100")
    if subsampling not in (0, 1, 2):
        raise ValueError(f"JPEG: subsampling {subsampling} (0 4:4:4, 1 4:2:2, 2 4:2:0)")
    if rows < 0:
        raise ValueError(f"JPEG: restart_marker_rows {rows} is negative")
    across = 2 if channels == 3 and subsampling else 1
    mcus_per_row = ((int(width) + 7) // 8 + across - 1) // across
    if rows * mcus_per_row > 65535:
        raise ValueError(f"JPEG: restart_marker_rows {rows} x {mcus_per_row} MCUs per row passes the 65535 MCUs of a restart interval")
    return quality, subsampling, rows, rows * mcus_per_row


def _jpeg_host(image: np.ndarray, **options: Any) -> bytes:
    """One image on the host with PIL: uint8 [H,W] or [H,W,1] (mode L) or [H,W,3] (RGB); `quality`, `subsampling`,
    `restart_marker_rows` as `JpegEncoder` takes them."""
    from PIL import Image

    arr = np.ascontiguousarray(image)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] not in (1, 3):
        raise ValueError(f"image: expected uint8 [H,W,C] with C 1 or 3, got {arr.dtype} {arr.shape}")
    quality, subsampling, rows, _ = _jpeg_options(arr.shape[2], arr.shape[0], arr.shape[1], **options)
    buf = io.BytesIO()
    if arr.shape[2] == 1:
        Image.fromarray(arr[:, :, 0]).save(buf, "JPEG", quality=quality, restart_marker_rows=rows)
    else:
        Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=rows)
    return buf.getvalue()


class JpegEncoder(_ImageEncoder):
    """`_ImageEncoder` for baseline JPEG, C = 1 (grey) or 3 (RGB) (`dad3d_jpeg_encode`, csrc/jpeg_encode.hip, DESIGN.md 4.20, two
    kernels), byte-equal to `Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling,
    restart_marker_rows=restart_marker_rows)`. `subsampling` 0 / 1 / 2 is 4:4:4 / 4:2:2 / 4:2:0; `None` is PIL's default for the
    mode. A restart marker per MCU row (`restart_marker_rows=1`) is what `jpeg_reader.JpegDecoder` reads in parallel. A flagged
    item goes to PIL, which writes the same bytes."""

    _CHANNELS = (1, 3)
    _LIMITS = "sides 1 .. 65535, at most 2^22 blocks"

    def __init__(self, height: int, width: int, channels: int, quality: int = 75, subsampling: Optional[int] = None,
                 restart_marker_rows: int = 0, device: Optional[int] = None):
        self.quality, self.subsampling, self.restart_marker_rows, self.restart_interval = _jpeg_options(
            int(channels), int(height), int(width), quality, subsampling, restart_marker_rows)
        self.options = {"quality": self.quality, "subsampling": self.subsampling, "restart_marker_rows": self.restart_marker_rows}
        super().__init__(height, width, channels, device)

    @staticmethod
    def _key_options(channels: int, height: int, width: int, **options: Any) -> tuple:
        return _jpeg_options(channels, height, width, **options)[:3]

    def _max_bytes(self) -> int:
        return self._lib.dad3d_jpeg_max_bytes(self.height, self.width, self.channels, self.subsampling)

    def _scratch_bytes_for(self, batch: int) -> int:
        return self._lib.dad3d_jpeg_encode_scratch_bytes(batch, self.height, self.width, self.channels, self.subsampling)

    def _launch(self, images: torch.Tensor, b: int, stream: int) -> int:
        return self._lib.dad3d_jpeg_encode(images.data_ptr(), b, self.height, self.width, self.channels, self.quality, self.subsampling,
                                           self.restart_interval, self._text.data_ptr(), self._text.stride(0), self._lengths.data_ptr(),
                                           self._flags.data_ptr(), self._scratch.data_ptr(), self._scratch.numel(), self.device, stream)

    @staticmethod
    def _host_encode(image: np.ndarray, **options: Any) -> bytes:
        return _jpeg_host(image, **options)


def _jpeg_encoder_for(images: torch.Tensor, **options: Any) -> JpegEncoder:
    return _encoder_for(JpegEncoder, images, **options)


def jpeg_batch(images: Any, **options: Any) -> List[bytes]:
    """`images [B,H,W,C]` uint8, C = 1 or 3 -> the bytes of one baseline JPEG file per image; `quality`, `subsampling` and
    `restart_marker_rows` as `JpegEncoder` takes them. A contiguous uint8 CUDA tensor is encoded on the GPU; anything else (a numpy
    array, a CPU tensor) by PIL on the host. Both write the same bytes."""
    return [bytes(x) for x in _image_files(JpegEncoder, images, "auto", **options)]


def save_jpeg_batch(images: Any, paths: Sequence[str], encoder: str = "auto", **options: Any) -> None:
    """`images [B,H,W,C]` uint8 -> one `.jpg` per image. A contiguous uint8 CUDA tensor with C in {1, 3} is encoded on the GPU
    (`JpegEncoder`; a flagged image is encoded here) and only the files cross to the host; a numpy array, a CPU tensor, a
    non-contiguous tensor or `encoder="host"` takes the host path: one copy of the pixels, PIL per image. The bytes are the same."""
    _save_image_files(JpegEncoder, images, paths, encoder, **options)


class _ZlibData(_DeviceText):
    def __init__(self, owner: "_ZlibCompressor", data: torch.Tensor, batch: int):
        super().__init__(owner, batch)
        self.data = data

    def _host_item(self, b: int) -> bytes:
        import zlib

        return zlib.compress(self.data[b].detach().cpu().numpy().tobytes(), 1)


class _ZlibCompressor(_TextBuffers):
    """The deflate of `PngEncoder` on plain byte rows `[B,n]`: one zlib stream per row (`dad3d_zlib_compress`)."""

    def __init__(self, n: int, device: int):
        super().__init__(device)
        self.n = int(n)
        worst = self._lib.dad3d_zlib_max_bytes(self.n)
        if worst == 0:
            raise ValueError(f"zlib_compress_batch: rows of {self.n} bytes (1 .. 2^31 - 1)")
        self.stride = (worst + 15) // 16 * 16

    def _scratch_bytes_for(self, batch: int) -> int:
        return self._lib.dad3d_zlib_scratch_bytes(batch, self.n)

    def compress(self, data: torch.Tensor) -> _ZlibData:
        b = data.shape[0]
        self.reserve(b)
        stream = torch.cuda.current_stream(self.torch_device).cuda_stream
        _lib.check(self._lib.dad3d_zlib_compress(data.data_ptr(), b, self.n, self._text.data_ptr(), self._text.stride(0),
                                                 self._lengths.data_ptr(), self._flags.data_ptr(), self._scratch.data_ptr(),
                                                 self._scratch.numel(), self.device, stream))
        return _ZlibData(self, data, b)


def zlib_compress_batch(data: torch.Tensor) -> List[bytes]:
    """`data [B,n]` uint8 on a GPU -> one zlib stream (RFC 1950) per row, from the deflate kernels of `PngEncoder`:
    `zlib.decompress(out[i]) == data[i]`."""
    if (not isinstance(data, torch.Tensor) or not data.is_cuda or data.dtype != torch.uint8 or data.ndim != 2 or not data.is_contiguous()
            or data.shape[1] < 1):
        raise ValueError(f"data: expected a contiguous uint8 CUDA tensor [B,n], n >= 1, got {getattr(data, 'dtype', type(data))} "
                         f"{tuple(getattr(data, 'shape', ()))} on {getattr(data, 'device', 'the host')}")
    if data.shape[0] == 0:
        return []
    return [bytes(x) for x in _ZlibCompressor(int(data.shape[1]), data.device.index).compress(data.detach()).to_host()]


def get_output_path(input_image_path: str, outputs_folder: str, type_of_output: str, extension: str) -> str:
    """demo_utils.py:156-163: `<outputs_folder>/<stem>_<type_of_output><extension>`."""
    stem = os.path.splitext(os.path.basename(input_image_path))[0]
    return os.path.join(outputs_folder, f"{stem}_{type_of_output}{extension}")
