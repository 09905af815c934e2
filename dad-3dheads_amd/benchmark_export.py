"""Wire format of the DAD-3DHeads accuracy benchmark, downstream of the decode.

A submission is one JSON object `{item_id: {"68_landmarks_2d": [[x, y]] * 68, "N_landmarks_3d": [[x, y, z]] * N,
"7_landmarks_3d": [[x, y, z]] * 7, "rotation_matrix": 3x3}}` (dad_3dheads_benchmark/README.md:78-95). The 68 3-D landmarks
are points ON the mesh: barycentric combinations of the corners of 68 fixed faces -- 17 contour points (row 0 of the
"dynamic" table: the reference always evaluates it at a zero pose) followed by 51 static points
(`get_68_landmarks`, dad_3dheads_benchmark/utils.py:29-117 == model_training/data/utils.py:120-206); the 7 alignment
landmarks are rows 36, 39, 42, 45, 33, 48, 54 of them (utils.py:143-151). Batched and device-resident here; the scoring side
(pose error, NME, Z5, Chamfer after Procrustes) is `evaluation.py`.

`submission_entry` + `write_submission` are the host path (`json.dump` of lists of floats). `SubmissionFormatter` and
`SubmissionWriter` make the same bytes on the GPU (`writers.JsonFormatter`, csrc/json_text.hip): only text crosses
to the host.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .synthetic import assets_dir

SEVEN_OF_68 = (36, 39, 42, 45, 33, 48, 54)  # get_7_landmarks_from_68's default (utils.py:145)


def embedding_path() -> str:
    """Packaged copy of the 68-landmark barycentric embedding (`face_idx`, `b_coords`); `DAD3D_LMK68_NPZ` overrides."""
    return os.environ.get("DAD3D_LMK68_NPZ") or os.path.join(assets_dir(), "lmk68_embedding.npz")


class Landmarks68:
    """`get_68_landmarks` for a batch of decoded meshes on any device: `[B,5023,3] -> [B,68,3]`."""

    def __init__(self, faces: np.ndarray, path: Optional[str] = None, device: Optional[torch.device] = None):
        with np.load(path or embedding_path()) as z:
            face_idx, b_coords = z["face_idx"].astype(np.int64), z["b_coords"].astype(np.float32)
        corners = np.asarray(faces).astype(np.int64)[face_idx]          # [68,3] vertex ids of the carrying faces
        self.corners = torch.from_numpy(corners).to(device)
        self.weights = torch.from_numpy(b_coords).to(device)            # [68,3]

    def __call__(self, vertices: Tensor) -> Tensor:
        single = vertices.ndim == 2
        v = vertices[None] if single else vertices
        assert v.shape[1:] == (5023, 3)  # utils.py:109-110
        c, w = self.corners.to(v.device), self.weights.to(v.device)
        tri = v[:, c, :]                                                 # [B,68,3 corners,3 xyz]
        # (verts * b_coords).sum(axis=1) of mesh_points_by_barycentric_coordinates, spelled out in its order
        out = tri[:, :, 0, :] * w[None, :, 0, None] + tri[:, :, 1, :] * w[None, :, 1, None] + tri[:, :, 2, :] * w[None, :, 2, None]
        return out[0] if single else out


def seven_landmarks(lmk68: Tensor, indices: Sequence[int] = SEVEN_OF_68) -> Tensor:
    return lmk68[..., list(indices), :]


def submission_entry(points_68_2d, vertices_3d: Tensor, lmk68_3d: Tensor, rotation_matrix) -> Dict[str, list]:
    """One value of the submission dict from one image's predictions (lists of lists of floats)."""
    to_list = lambda x: (x.detach().cpu() if isinstance(x, Tensor) else torch.as_tensor(np.asarray(x))).to(torch.float64).tolist()  # noqa: E731
    return {"68_landmarks_2d": to_list(points_68_2d), "N_landmarks_3d": to_list(vertices_3d),
            "7_landmarks_3d": to_list(seven_landmarks(lmk68_3d)), "rotation_matrix": to_list(rotation_matrix)}


def write_submission(path: str, entries: Mapping[str, Mapping[str, list]]) -> None:
    with open(path, "w") as f:
        json.dump({str(k): dict(v) for k, v in entries.items()}, f)


SUBMISSION_FLAG_INEXACT = 0x100  # ORed into an item's flags on the device: an input value is no float32, the host formats the item


class SubmissionFormatter:
    """`submission_entry` + `json.dumps` for a batch, on the GPU: `entries(...)[b]` equals
    `json.dumps(submission_entry(points_68_2d[b], vertices_3d[b], lmk68_3d[b], rotation_matrix[b])).encode()`.

    The four fields are gathered into the formatter's float32 staging buffer `[B, 68*2 + N*3 + 7*3 + 9]` on the device (the
    buffers grow to the largest batch seen, then stay). `submission_entry` prints every value as a double; what the kernel prints
    is a float32 widened to double, so a value that is no float32 must not take the device path: an integer tensor is cast on the
    device and `|v| > 2^24` ORs `SUBMISSION_FLAG_INEXACT` into the item's flag there, a float64 tensor does the same where the
    cast changes the value. A flagged item (also one with NaN or an infinity) is formatted by `submission_entry` on the host."""

    def __init__(self, n_vertices: int = 5023, device: Optional[int] = None):
        from . import writers

        self.n_vertices = int(n_vertices)
        self.template = writers.JsonTemplate.from_structure({"68_landmarks_2d": (68, 2), "N_landmarks_3d": (self.n_vertices, 3),
                                                             "7_landmarks_3d": (7, 3), "rotation_matrix": (3, 3)})
        self.formatter = writers.JsonFormatter(self.template, device=device)
        self.torch_device = self.formatter.torch_device
        self._seven_index = torch.tensor(SEVEN_OF_68, dtype=torch.int64, device=self.torch_device)
        self._capacity = 0

    def reserve(self, batch: int) -> None:
        batch = max(int(batch), 1)
        self.formatter.reserve(batch)
        if batch > self._capacity:
            self._capacity = batch
            self._inexact = torch.zeros(batch, dtype=torch.int32, device=self.torch_device)

    def _stage(self, field: Any, columns: Tensor, inexact: Tensor) -> None:
        t = field if isinstance(field, Tensor) else torch.as_tensor(np.asarray(field))
        t = t.detach().to(self.torch_device).reshape(columns.shape)
        columns.copy_(t)  # the cast to float32 happens on the device
        if t.dtype in (torch.float32, torch.float16, torch.bfloat16):
            return
        if t.dtype.is_floating_point:
            changed = (columns.to(t.dtype) != t).any(dim=1)
        else:
            changed = (t.abs() > 2 ** 24).any(dim=1)
        inexact.bitwise_or_(changed.to(torch.int32) * SUBMISSION_FLAG_INEXACT)

    def format(self, points_68_2d, vertices_3d, lmk68_3d, rotation_matrix):
        """Gather, cast and launch on the current stream; no wait. -> `writers.JsonText`."""
        b, n = int(vertices_3d.shape[0]), self.n_vertices
        assert tuple(vertices_3d.shape[1:]) == (n, 3) and tuple(points_68_2d.shape) == (b, 68, 2)
        assert tuple(lmk68_3d.shape) == (b, 68, 3) and tuple(rotation_matrix.shape) == (b, 3, 3)
        self.reserve(b)
        staged, inexact = self.formatter.staging(b), self._inexact[:b]
        inexact.zero_()
        lmk = lmk68_3d if isinstance(lmk68_3d, Tensor) else torch.as_tensor(np.asarray(lmk68_3d))
        seven = torch.index_select(lmk.detach().to(self.torch_device), 1, self._seven_index)
        cuts = np.cumsum([0, 68 * 2, n * 3, 7 * 3, 9])
        for field, lo, hi in zip((points_68_2d, vertices_3d, seven, rotation_matrix), cuts[:-1], cuts[1:]):
            self._stage(field, staged[:, lo:hi], inexact)

        def host_item(i: int) -> bytes:
            return json.dumps(submission_entry(points_68_2d[i], vertices_3d[i], lmk68_3d[i], rotation_matrix[i])).encode("ascii")

        return self.formatter.format(staged, host_item=host_item, extra_flags=inexact)

    def entries(self, points_68_2d, vertices_3d, lmk68_3d, rotation_matrix) -> List[bytes]:
        return [bytes(x) for x in self.format(points_68_2d, vertices_3d, lmk68_3d, rotation_matrix).to_host()]


class SubmissionWriter:
    """Writes a submission file batch by batch: the bytes of `write_submission(path, {id: submission_entry(...)})` over the same
    rows in the same order (ids unique, as the keys of that dict are).

        with SubmissionWriter(path) as w:
            for ids, points, vertices, lmk68, rotation in batches:
                w.add(ids, points, vertices, lmk68, rotation)

    Two formatters take turns: `add` launches the format and the text copy of its batch on a side stream, then writes the batch
    before it to the file while that copy runs."""

    def __init__(self, path: str, n_vertices: int = 5023, device: Optional[int] = None):
        self.path = path
        self._pair = [SubmissionFormatter(n_vertices, device), SubmissionFormatter(n_vertices, device)]
        self._dev = self._pair[0].torch_device
        self._side = torch.cuda.Stream(device=self._dev)
        self._pending = None
        self._batches, self._written = 0, 0
        self._file = None

    def __enter__(self) -> "SubmissionWriter":
        self._file = open(self.path, "wb")
        self._file.write(b"{")
        return self

    def add(self, ids: Sequence[Any], points_68_2d, vertices_3d, lmk68_3d, rotation_matrix) -> None:
        assert self._file is not None and len(ids) == int(vertices_3d.shape[0])
        current = torch.cuda.current_stream(self._dev)
        self._side.wait_stream(current)
        with torch.cuda.stream(self._side):
            text = self._pair[self._batches % 2].format(points_68_2d, vertices_3d, lmk68_3d, rotation_matrix)
            text.begin_host_copy()
        current.wait_stream(self._side)  # the caller may reuse its tensors: the gather has read them
        self._batches += 1
        previous, self._pending = self._pending, (list(ids), text)
        if previous is not None:
            self._write(previous)

    def _write(self, batch) -> None:
        ids, text = batch
        with torch.cuda.stream(self._side):
            blocks = text.to_host()
        for key, block in zip(ids, blocks):
            self._file.write((b", " if self._written else b"") + json.dumps(str(key)).encode("ascii") + b": ")
            self._file.write(block)
            self._written += 1

    def __exit__(self, exc_type, exc, tb) -> None:
        try:
            if exc_type is None:
                if self._pending is not None:
                    self._write(self._pending)
                self._file.write(b"}")
        finally:
            self._pending = None
            self._file.close()
            self._file = None
