"""On-disk formats downstream of the decode: the `.obj` mesh text and the FLAME-parameter JSON of the
reference's demo (`demo_utils.py:106-153`). Same bytes as `MeshSaver` / `JsonSaver` write; the batch variants format a
whole batch of decoded meshes with the constant face block rendered once.

The vertex block of a float32 CUDA batch is formatted on the GPU (`ObjFormatter`, csrc/obj_text.hip: the same bytes from 64-bit
integer arithmetic); a mesh that holds a value outside the kernel's domain (NaN, inf, |x| >= 2^37) is flagged
there and formatted by `_vertex_block` here. The JSON writers stay on the host (`json.dump` prints the shortest round-trip
form of a double, another algorithm), as do the face block (a constant) and `MeshSaver.__call__` for one host mesh.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import os
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .flame import FLAME_CONSTS, FlameParams


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


class ObjText:
    """What `ObjFormatter.format` returns: the vertex text of `batch` meshes in HBM. Mesh b's bytes are
    `text[b, :lengths[b]]` (byte offset `b * stride` of the buffer); `flags[b] != 0` marks a mesh the kernel left to the host.
    The buffers belong to the formatter: they hold this batch until its next `format`."""

    def __init__(self, formatter: "ObjFormatter", vertices: torch.Tensor, batch: int):
        self.formatter, self.vertices, self.batch = formatter, vertices, batch
        self.text, self.stride = formatter._text[:batch], formatter.stride
        self.lengths, self.flags = formatter._lengths[:batch], formatter._flags[:batch]
        self.offsets = [b * self.stride for b in range(batch)]
        self._copy: Optional[Tuple[np.ndarray, np.ndarray, int, torch.cuda.Event]] = None

    def begin_host_copy(self) -> None:
        """Waits for the lengths and flags (one small copy), then enqueues the copy of the text that exists -- `batch` rows of the
        longest mesh's length, not of the worst-case stride -- into the formatter's pinned buffer, without waiting for it."""
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
        """The vertex block of every mesh as bytes on the host: a `memoryview` into the formatter's pinned buffer (valid until
        its next `to_host`), or `bytes` from the host formatter for a flagged mesh."""
        self.begin_host_copy()
        lengths, flags, width, done = self._copy
        done.synchronize()
        host = memoryview(self.formatter._host.numpy())
        out: List[Any] = []
        for b in range(self.batch):
            if flags[b]:
                out.append(_vertex_block(self.vertices[b].detach().cpu().numpy()).encode("ascii"))
            else:
                out.append(host[b * width : b * width + int(lengths[b])])
        return out


class ObjFormatter:
    """The `v %.8f %.8f %.8f` lines of a batch of meshes, formatted on the GPU (`dad3d_obj_format_vertices`).

    `reserve(batch)` allocates the device text buffer (`batch` rows of the worst case, 71 bytes per line), lengths, flags,
    scratch and one pinned host buffer; `format(vertices)` launches on the current stream with no allocation and no sync once
    the batch fits (capturable in a graph); `ObjText.to_host()` brings the bytes over. `faces` (0-based, as `save_obj_batch`
    takes them) gives `face_text`, the constant block behind every mesh's vertices."""

    def __init__(self, n_verts: int, faces: Optional[np.ndarray] = None, device: Optional[int] = None):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.torch_device = torch.device("cuda", self.device)
        self.n_verts = int(n_verts)
        self.stride = (self.n_verts * _lib.OBJ_MAX_LINE_BYTES + 15) // 16 * 16
        self.face_text = b"" if faces is None else _face_block(np.asarray(faces) + 1.0).encode("ascii")
        self.capacity = 0

    def reserve(self, batch: int) -> None:
        batch = max(int(batch), 1)
        if batch <= self.capacity:
            return
        dev = self.torch_device
        self.capacity = batch
        self._text = torch.empty((batch, max(self.stride, 16)), dtype=torch.uint8, device=dev)
        self._meta = torch.zeros(12 * batch, dtype=torch.uint8, device=dev)  # lengths int64 [batch] | flags int32 [batch]
        self._lengths, self._flags = self._meta[: 8 * batch].view(torch.int64), self._meta[8 * batch :].view(torch.int32)
        self._scratch_bytes = int(self._lib.dad3d_obj_format_scratch_bytes(batch, self.n_verts))
        self._scratch = torch.empty(max(self._scratch_bytes, 8), dtype=torch.uint8, device=dev)
        self._meta_host = torch.empty(12 * batch, dtype=torch.uint8).pin_memory()
        self._host = torch.empty(batch * max(self.stride, 16), dtype=torch.uint8).pin_memory()

    def format(self, vertices: torch.Tensor) -> ObjText:
        if (not isinstance(vertices, torch.Tensor) or vertices.device != self.torch_device or vertices.dtype != torch.float32
                or not vertices.is_contiguous() or vertices.ndim != 3 or tuple(vertices.shape[1:]) != (self.n_verts, 3)):
            raise ValueError(f"vertices: expected a contiguous float32 tensor [B,{self.n_verts},3] on {self.torch_device}, got "
                             f"{getattr(vertices, 'dtype', type(vertices))} {tuple(getattr(vertices, 'shape', ()))} on "
                             f"{getattr(vertices, 'device', 'the host')}"
                             + ("" if not isinstance(vertices, torch.Tensor) or vertices.is_contiguous() else " (not contiguous)"))
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
    for block, path in zip(blocks, paths):
        with open(path, "wb") as f:
            f.write(block)
            f.write(face_text)


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


def flame_params_batch(params: torch.Tensor, constants: Dict[str, int] = FLAME_CONSTS) -> List[Dict[str, List[float]]]:
    """`params [B,413]` -> the per-image dictionaries `get_flame_params` produces."""
    fp = FlameParams.from_3dmm(params.detach().cpu(), constants)
    fields = {k: v.tolist() for k, v in vars(fp).items()}
    return [{k: rows[i] for k, rows in fields.items()} for i in range(params.shape[0])]


def get_output_path(input_image_path: str, outputs_folder: str, type_of_output: str, extension: str) -> str:
    """demo_utils.py:156-163: `<outputs_folder>/<stem>_<type_of_output><extension>`."""
    stem = os.path.splitext(os.path.basename(input_image_path))[0]
    return os.path.join(outputs_folder, f"{stem}_{type_of_output}{extension}")
