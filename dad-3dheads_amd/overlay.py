"""The demo's overlays on the GPU: `demo_utils.py`'s `draw_points`, `draw_landmarks`, `draw_3d_landmarks`, `draw_mesh` and `draw_pose`
for batches of uint8 images that stay on the device (csrc/overlay.hip; the outputs `68_landmarks`, `191_landmarks`, `445_landmarks`,
`head_mesh`, `face_mesh` and `pose` of the reference's demo.py), and `draw_heads`: the heads of `predict_boxes` as shaded or PNCC surfaces
in their frames, all frames and heads in one raster chain (csrc/sim3dr_frames.hip).

`images` is a CUDA uint8 tensor `[B,H,W,3]`, one image `[H,W,3]`, or a list of `[H,W,3]` tensors of any sizes (one launch per
distinct shape). The result has the form of the input and is a new tensor: an input is only drawn into when it is passed as `out=`.
`predictions` is what the predictor returns, in either form: the list of per-image dicts of `predict_batch` / `predict_files`
(`device_outputs=True` or not; host values are uploaded) or the one dict of batched tensors of `predict_tensor`.

Pinned to the reference: which vertices and index lists are drawn, the `astype(int)` truncation, the colours, radii, thickness and
arrow geometry, the draw order and what each function returns. NOT pinned: the pixels of a stroke. cv2 is not installed anywhere this
project runs, so the stroke rules are this project's own, in exact integer arithmetic (include/dad3d.h); the kernels
equal tests/overlay_restatement.py to the bit. Left out: `addWeighted` (the reference computes the blend and returns the unblended
image), text, and the training mixin's panels.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .flame import FLAME_CONSTS, FlameParams
from .synthetic import load_static

POINT_COLOR = (255, 0, 0)  # demo_utils.py:15-16
EDGE_COLOR = (39, 48, 218)
POSE_COLORS = ((0, 0, 255), (0, 255, 0), (255, 0, 0))  # demo_utils.py:90-92
SUBSETS = ("191", "445", "565")
RPY = namedtuple("RPY", ["roll", "pitch", "yaw"])  # model_training/model/flame.py

Images = Union[Tensor, Sequence[Tensor]]
Predictions = Union[Dict[str, object], Sequence[Dict[str, object]]]


# -- images: validation, grouping by shape, the launches ----------------------------------------------------------------------------
def _image_list(images: Images) -> Tuple[List[Tensor], str]:
    """The images as a list of [H,W,3] views, and the form of the input: "batch", "single" or "list"."""
    if isinstance(images, Tensor):
        form = "batch" if images.ndim == 4 else "single"
        items = list(images.unbind(0)) if images.ndim == 4 else [images]
        if images.ndim not in (3, 4):
            raise ValueError(f"images: expected uint8 [B,H,W,3] or [H,W,3], got shape {tuple(images.shape)}")
    else:
        form, items = "list", list(images)
    for t in items:
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("images: expected uint8 tensors [H,W,3], got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if not (1 <= t.shape[0] <= _lib.OVERLAY_MAX_COORD and 1 <= t.shape[1] <= _lib.OVERLAY_MAX_COORD):
            raise ValueError(f"images: {t.shape[0]} x {t.shape[1]} is outside 1 .. {_lib.OVERLAY_MAX_COORD}")
    return items, form


def _color(color) -> int:
    c = [int(v) for v in color]
    if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
        raise ValueError(f"color: expected three values in 0 .. 255, got {color!r}")
    return c[0] | c[1] << 8 | c[2] << 16


def _draw(images: Images, out: Optional[Images], tables_for: Callable[[List[int], int, int, torch.device], Tensor],
          launch: Callable[[Tensor, Tensor, Tensor, int, int], None]):
    """Run `launch(src, dst, table, h, w)` once per distinct image shape. `tables_for(indices, h, w, device)` gives the float32
    point table [len(indices),P,2] of those images on `device`."""
    items, form = _image_list(images)
    for t in items:
        if not t.is_cuda:
            raise ValueError("images: expected CUDA tensors (the overlays are drawn on the GPU; there is no CPU fallback)")
    if form != "list":
        src = images.contiguous()
        src4 = src if form == "batch" else src[None]
        if out is None:
            out = torch.empty_like(src)
        if not isinstance(out, Tensor) or out.shape != src.shape or out.dtype != torch.uint8 or out.device != src.device or not out.is_contiguous():
            raise ValueError("out: expected a contiguous uint8 tensor of the images' shape on their device")
        if out is images and src is not images:
            raise ValueError("out: drawing in place needs contiguous images")
        if src4.shape[0]:
            h, w = src4.shape[1:3]
            launch(src4, out if form == "batch" else out[None], tables_for(list(range(src4.shape[0])), h, w, src.device), h, w)
        return out
    groups: Dict[Tuple[int, int, torch.device], List[int]] = {}
    for i, t in enumerate(items):
        groups.setdefault((t.shape[0], t.shape[1], t.device), []).append(i)
    results: List[Optional[Tensor]] = [None] * len(items)
    for (h, w, dev), idx in groups.items():
        stacked = torch.stack([items[i] for i in idx])  # a copy: the inputs stay as they were
        launch(stacked, stacked, tables_for(idx, h, w, dev), h, w)
        for k, i in enumerate(idx):
            results[i] = stacked[k]
    if out is None:
        return results
    if len(out) != len(items):
        raise ValueError(f"out: {len(out)} tensors for {len(items)} images")
    for o, r in zip(out, results):
        o.copy_(r)
    return out


def _stream(t: Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _launch_segments(src: Tensor, dst: Tensor, table: Tensor, edges: Tensor, colors: Optional[Tensor], color: int, thickness: int):
    b, h, w = src.shape[:3]
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] == b and table.shape[2] == 2 and table.device == src.device
    assert edges.dtype == torch.int32 and edges.is_contiguous() and edges.device == src.device
    _lib.check(_lib.load().dad3d_overlay_segments(src.data_ptr(), dst.data_ptr(), b, h, w, table.data_ptr(), table.shape[1], edges.data_ptr(),
                                                  edges.shape[0], colors.data_ptr() if colors is not None else None, color, thickness,
                                                  src.device.index, _stream(src)))


def _launch_discs(src: Tensor, dst: Tensor, table: Tensor, index: Optional[Tensor], radius: int, color: int):
    b, h, w = src.shape[:3]
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] == b and table.shape[2] == 2 and table.device == src.device
    n = index.shape[0] if index is not None else table.shape[1]
    _lib.check(_lib.load().dad3d_overlay_discs(src.data_ptr(), dst.data_ptr(), b, h, w, table.data_ptr(), table.shape[1],
                                               index.data_ptr() if index is not None else None, n, radius, color, src.device.index,
                                               _stream(src)))


# -- predictions: either form -> one tensor per field -------------------------------------------------------------------------------
def _field(predictions: Predictions, key: str, n_images: int, row_dims: int) -> Tensor:
    """`predictions[key]` of every image as one tensor [n_images, ...] (`row_dims` dimensions per image), where it lies."""
    dicts = [predictions] if isinstance(predictions, dict) else list(predictions)
    parts = []
    for d in dicts:
        t = d[key] if isinstance(d[key], Tensor) else torch.as_tensor(np.asarray(d[key]))
        if t.ndim == row_dims:
            t = t[None]
        if t.ndim != row_dims + 1:
            raise ValueError(f"predictions[{key!r}]: expected {row_dims} or {row_dims + 1} dimensions, got shape {tuple(t.shape)}")
        parts.append(t)
    t = parts[0] if len(parts) == 1 else torch.cat([p.to(parts[0].device) for p in parts])
    if t.shape[0] != n_images:
        raise ValueError(f"predictions[{key!r}] holds {t.shape[0]} items for {n_images} images")
    return t


def _table(points, n_images: int) -> Tensor:
    """A point table [n_images,P,2] (tensor, array or list of [P,2]) as float32, where it lies."""
    if isinstance(points, (list, tuple)):
        points = torch.stack([p if isinstance(p, Tensor) else torch.as_tensor(np.asarray(p)) for p in points])
    t = points if isinstance(points, Tensor) else torch.as_tensor(np.asarray(points))
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] < 2 or t.shape[0] != n_images:
        raise ValueError(f"points: expected [{n_images},P,2], got shape {tuple(t.shape)}")
    return t[..., :2]


def _tables_from(table: Tensor):
    def tables_for(idx: List[int], h: int, w: int, device: torch.device) -> Tensor:
        t = table if idx == list(range(table.shape[0])) else table[torch.as_tensor(idx, device=table.device)]
        return t.to(device, torch.float32).contiguous()
    return tables_for


# -- several heads per frame ---------------------------------------------------------------------------------------------------------
def _by_frame(draw: Callable, predictions: Predictions, images: Images, image_index, out: Optional[Images], **kwargs):
    """`draw(predictions, images, ...)` for predictions that name their frames: prediction k is drawn into `images[image_index[k]]`,
    the heads of one frame in the order they come. Round r draws the r-th head of every frame that has one into the running
    images, on the kernels `draw` launches anyway, so the bytes are those of one call per head on the running image (a loop over
    the reference's demo_utils). A frame without heads is copied."""
    items, form = _image_list(images)
    if isinstance(predictions, dict):
        raise ValueError("image_index: expected the list of per-head dicts that predict_boxes returns")
    dicts = list(predictions)
    index = np.asarray(image_index.cpu() if isinstance(image_index, Tensor) else image_index).reshape(-1).astype(np.int64)  # a tensor: one wait
    if len(index) != len(dicts):
        raise ValueError(f"image_index: {len(index)} entries for {len(dicts)} predictions")
    if len(index) and not (0 <= index.min() and index.max() < len(items)):
        raise ValueError(f"image_index: values outside 0 .. {len(items) - 1}")
    heads: List[List[int]] = [[] for _ in items]
    for k, i in enumerate(index):
        heads[int(i)].append(k)
    running = [t.clone() for t in items]
    for r in range(max((len(h) for h in heads), default=0)):
        frames = [i for i, h in enumerate(heads) if len(h) > r]
        drawn = draw([dicts[heads[i][r]] for i in frames], [running[i] for i in frames], **kwargs)
        for i, t in zip(frames, drawn):
            running[i] = t
    result = torch.stack(running) if form == "batch" else running[0] if form == "single" else running
    if out is None:
        return result
    if form == "list":
        if len(out) != len(items):
            raise ValueError(f"out: {len(out)} tensors for {len(items)} images")
        for o, t in zip(out, running):
            o.copy_(t)
    else:
        out.copy_(result)
    return out


def _head_index(dicts: Sequence[Dict[str, object]], image_index, device: torch.device):
    """The frame number of every head for `Mesh.rasterize_frames`: a CUDA int32 tensor where the values lie on the device (never
    read here), a host array otherwise. `image_index=None`: the `"image_index"` of the dicts."""
    values = [d["image_index"] for d in dicts] if image_index is None else image_index
    if isinstance(values, Tensor):
        return values.to(device, torch.int32).reshape(-1) if values.is_cuda else values.numpy().reshape(-1).astype(np.int32)
    values = list(values)
    if values and all(isinstance(v, Tensor) and v.is_cuda for v in values):
        return torch.stack([v.reshape(()) for v in values]).to(device, torch.int32)
    return np.asarray([int(v) for v in values], dtype=np.int32)


_renderers: Dict[Tuple[int, str], object] = {}  # (id of the head mesh, mode) -> PNCCEstimator | Mesh; the head mesh is kept alive with it


def draw_heads(predictions: Predictions, frames: Images, mode: str = "shaded", image_index=None, out: Optional[Images] = None,
               head_mesh=None, textures=None, creator=None, mapping: str = "bilinear"):
    """The heads of `predict_boxes` / `predict_files(.., boxes=)` drawn into their frames as surfaces: `mode="shaded"` the whole FLAME
    mesh under RenderPipeline's default light, `mode="pncc"` the ear-less face subset in its colour codes (pncc_estimator.py). The
    dicts' `3dmm_params` are already in frame coordinates; they are stacked and decoded once (`proj`, z flipped, as
    `PNCCEstimator.render_batch` does), and all heads of all frames go through one `Mesh.render_frames` / `rasterize_frames` chain:
    head k into `frames[image_index[k]]`, a later head of a frame over an earlier one, as a loop over `Sim3DR.rasterize(.., bg=frame)`
    paints them. `image_index=None`: the dicts' own. A head whose index names no frame is not drawn. With device values nothing is
    read on the host. `frames` as for the other overlays; the result has their form and is a copy unless `out=` is given (`out` may be
    `frames` itself). `head_mesh`: the predictor's `HeadMesh` (None: a new one, which needs the FLAME model file).
    `mode="textured"`: every head with its own texture, `textures` a `[N,S,S,3]` tensor (one shared `[S,S,3]` works too) or a
    `uv_texture.TextureAccumulator` (slot k for head k), through `creator.render_frames` (`creator`: the `UVTextureCreator` that holds
    the texture coordinates; None: the accumulator's), sampled `mapping="bilinear"` or `"nearest"`."""
    if mode not in ("shaded", "pncc", "textured"):
        raise ValueError(f"mode: 'shaded', 'pncc' or 'textured', got {mode!r}")
    if mode != "textured" and (textures is not None or creator is not None):
        raise ValueError(f"textures / creator: only with mode='textured', got mode={mode!r}")
    if mode == "textured":
        if textures is None:
            raise ValueError("mode='textured' needs textures= (a tensor or a TextureAccumulator)")
        if creator is None:
            creator = getattr(textures, "creator", None)
        if creator is None:
            raise ValueError("mode='textured' with a texture tensor needs creator= (the UVTextureCreator with the texture coordinates)")
    items, form = _image_list(frames)
    for t in items:
        if not t.is_cuda:
            raise ValueError("frames: expected CUDA tensors (the heads are drawn on the GPU; there is no CPU fallback)")
    if isinstance(predictions, dict):
        raise ValueError("predictions: expected the list of per-head dicts that predict_boxes returns")
    dicts = list(predictions)
    if out is None:
        target = frames.clone() if form != "list" else [t.clone() for t in items]
    else:
        target = out
        if form == "list":
            if len(out) != len(items):
                raise ValueError(f"out: {len(out)} tensors for {len(items)} frames")
            for o, t in zip(out, items):
                if o.shape != t.shape or o.dtype != torch.uint8 or o.device != t.device:
                    raise ValueError("out: expected uint8 tensors of the frames' shapes on their device")
                if o is not t:
                    o.copy_(t)
        else:
            if not isinstance(out, Tensor) or out.shape != frames.shape or out.dtype != torch.uint8 or out.device != frames.device:
                raise ValueError("out: expected a uint8 tensor of the frames' shape on their device")
            if out is not frames:
                out.copy_(frames)
    if not dicts or not items:
        return target
    device = items[0].device
    if mode == "textured":
        params = _field(dicts, "3dmm_params", len(dicts), 1).to(device, torch.float32).contiguous()
        index = _head_index(dicts, image_index, device)
        if len(index) != len(dicts):
            raise ValueError(f"image_index: {len(index)} entries for {len(dicts)} predictions")
        creator.render_frames(params, textures, target if form != "single" else [target], index, mapping=mapping, mutate=False)
        return target
    if head_mesh is None:
        from .head_mesh import HeadMesh
        head_mesh = HeadMesh(device=device.index)
    params = _field(dicts, "3dmm_params", len(dicts), 1).to(device, torch.float32).contiguous()
    index = _head_index(dicts, image_index, device)
    if len(index) != len(dicts):
        raise ValueError(f"image_index: {len(index)} entries for {len(dicts)} predictions")
    draw_into = target if form == "list" else target if form == "batch" else [target]
    key = (id(head_mesh), mode)
    if mode == "pncc":
        if key not in _renderers:
            from .pncc import PNCCEstimator
            _renderers[key] = PNCCEstimator(head_mesh=head_mesh)
        _renderers[key].render_frames(params, draw_into, index, mutate=False)
    else:
        flame = head_mesh.flame
        if key not in _renderers:
            from .Sim3DR.mesh import Mesh
            _renderers[key] = (Mesh(np.ascontiguousarray(np.asarray(flame.faces), dtype=np.int32),
                                    int(np.asarray(flame.flame_model.v_template).shape[0]), device=flame.device_index), head_mesh)
        verts = flame.decode(params, proj=True, to_2d=False, flip_z=True, mutate=False)["proj"]
        _renderers[key][0].render_frames(draw_into, verts, index)
    return target


# -- the reference's surface --------------------------------------------------------------------------------------------------------
def default_radius(h: int, w: int) -> int:
    return max(1, int(min(h, w) * 0.005))  # demo_utils.py:26


def draw_points(images: Images, points, radius: Optional[int] = None, color=POINT_COLOR, index: Optional[Tensor] = None,
                out: Optional[Images] = None):
    """demo_utils.py:22-29: a filled disc of `radius` (None: `max(1, int(min(h, w) * 0.005))`) at every point, truncated toward zero.
    `points` [B,P,2] (tensor or array, any numeric dtype; a list of [P,2]); `index` an int32 CUDA tensor [K] picks points."""
    items, _ = _image_list(images)
    rgb = _color(color)
    if radius is not None and not 1 <= int(radius) <= _lib.OVERLAY_MAX_COORD:
        raise ValueError(f"radius: {radius} is outside 1 .. {_lib.OVERLAY_MAX_COORD}")
    table = _table(points, len(items))

    def launch(src, dst, tab, h, w):
        _launch_discs(src, dst, tab, index, int(radius) if radius is not None else default_radius(h, w), rgb)

    return _draw(images, out, _tables_from(table), launch)


def draw_landmarks(predictions: Predictions, images: Images, out: Optional[Images] = None, image_index=None):
    """demo_utils.py:32-34: the 68 predicted 2-D landmarks `predictions["points"]`. With `image_index` (one frame number per
    prediction, as `predict_boxes` returns them) prediction k is drawn into `images[image_index[k]]`, several heads of a frame in order."""
    if image_index is not None:
        return _by_frame(draw_landmarks, predictions, images, image_index, out)
    items, _ = _image_list(images)
    return draw_points(images, _field(predictions, "points", len(items), 2), out=out)


_index_cache: Dict[Tuple[str, torch.device], Tensor] = {}


@functools.lru_cache(maxsize=None)
def _subset_ids(subset: str) -> np.ndarray:
    ids = np.asarray(load_static()[f"lmk_{subset}"]).astype(np.int32)
    ids.setflags(write=False)  # cached: one array for every caller
    return ids


def landmark_indices(subset: str) -> np.ndarray:
    """The vertex ids of a 3-D landmark subset, from the packaged `flame_static.npz`: "191", "445" (the canonical list) or "565"
    (what the reference's `demo.py 445_landmarks` draws: every file of the keypoints_445 directory). Any other value raises
    ValueError (demo_utils.py:38-40 builds the error and forgets to raise it)."""
    if not isinstance(subset, str) or subset not in SUBSETS:
        raise ValueError(f"Invalid keypoints subset provided: {subset!r}.\nAvailable options are: {', '.join(SUBSETS)}")
    return _subset_ids(subset)


def draw_3d_landmarks(predictions: Predictions, images: Images, subset: str = "191", out: Optional[Images] = None, image_index=None):
    """demo_utils.py:37-47: discs at the projected vertices of a landmark subset. `image_index`: as in `draw_landmarks`."""
    if image_index is not None:
        landmark_indices(subset)
        return _by_frame(draw_3d_landmarks, predictions, images, image_index, out, subset=subset)
    ids = landmark_indices(subset)
    items, _ = _image_list(images)
    verts = _field(predictions, "projected_vertices", len(items), 2)
    rgb = _color(POINT_COLOR)

    def launch(src, dst, tab, h, w):
        key = (subset, src.device)
        if key not in _index_cache:
            _index_cache[key] = torch.from_numpy(ids.copy()).to(src.device)
        _launch_discs(src, dst, tab, _index_cache[key], default_radius(h, w), rgb)

    return _draw(images, out, _tables_from(verts[..., :2]), launch)


def mesh_edges(faces=None, subset=None) -> np.ndarray:
    """The sorted unique edges (lower vertex id first) of the triangles `faces` [F,3] (None: the packaged FLAME faces), int32 [E,2].
    `subset`: vertex ids; only edges with both ends among them are kept. These are NOT the reference's `head_edges.npy` /
    `face_edges.npy`, which cannot be derived from the faces; they serve a caller without a checkout of the reference."""
    f = np.asarray(load_static()["faces"] if faces is None else faces)
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces: expected an integer array [F,3], got {f.dtype} {f.shape}")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    e = np.unique(np.sort(e, axis=1), axis=0)
    if subset is not None:
        keep = np.isin(e, np.asarray(subset).astype(np.int64)).all(1)
        e = e[keep]
    return np.ascontiguousarray(e, dtype=np.int32)


def load_edges(edges) -> np.ndarray:
    """`edges`: an integer array [E,2] or the path of the reference's `head_edges.npy` / `face_edges.npy` -> int32 [E,2]."""
    e = np.load(edges) if isinstance(edges, (str, bytes)) or hasattr(edges, "__fspath__") else np.asarray(edges)
    if e.ndim != 2 or e.shape[1] != 2 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"edges: expected an integer array [E,2], got {e.dtype} {e.shape}")
    return np.ascontiguousarray(e, dtype=np.int32)


def draw_segments(images: Images, points, edges, color=EDGE_COLOR, colors=None, thickness: int = 0, out: Optional[Images] = None):
    """Segment e joins `points[b, edges[e, 0]]` and `points[b, edges[e, 1]]`, drawn in the list's order: anti-aliased and one pixel
    wide (`thickness=0`) or solid (1 .. 255). `edges`: what `load_edges` takes, or an int32 CUDA tensor [E,2] (used as it is; the
    kernel skips an index outside the table). `colors` [E,3] uint8 gives every segment its own colour."""
    items, _ = _image_list(images)
    rgb = _color(color)
    if not 0 <= int(thickness) <= 255:
        raise ValueError(f"thickness: {thickness} is outside 0 (anti-aliased) .. 255")
    table = _table(points, len(items))
    on_device = isinstance(edges, Tensor) and edges.is_cuda
    if on_device:
        if edges.dtype != torch.int32 or edges.ndim != 2 or edges.shape[1] != 2 or not edges.is_contiguous():
            raise ValueError(f"edges: a device list must be a contiguous int32 tensor [E,2], got {edges.dtype} {tuple(edges.shape)}")
    else:
        host = load_edges(edges.numpy() if isinstance(edges, Tensor) else edges)
        if host.size and (host.min() < 0 or host.max() >= table.shape[1]):
            raise ValueError(f"edges: vertex ids {int(host.min())} .. {int(host.max())} outside the {table.shape[1]} points")
    n_edges = edges.shape[0] if on_device else host.shape[0]
    if colors is not None:
        colors = colors if isinstance(colors, Tensor) else torch.as_tensor(np.asarray(colors))
        if colors.dtype != torch.uint8 or tuple(colors.shape) != (n_edges, 3):
            raise ValueError(f"colors: expected uint8 [{n_edges},3], got {colors.dtype} {tuple(colors.shape)}")

    def launch(src, dst, tab, h, w):
        e = edges.to(src.device) if on_device else torch.from_numpy(host).to(src.device)
        c = colors.to(src.device).contiguous() if colors is not None else None
        _launch_segments(src, dst, tab, e, c, rgb, int(thickness))

    return _draw(images, out, _tables_from(table), launch)


def draw_mesh(predictions: Predictions, images: Images, edges, out: Optional[Images] = None, image_index=None):
    """demo_utils.py:50-65: the mesh's edges over `projected_vertices`, anti-aliased, EDGE_COLOR, in the list's order. Returns the
    line image, as the reference does (its `addWeighted` blend goes into a copy that is never returned; none is computed here).
    `edges`: the path of the reference's `head_edges.npy` / `face_edges.npy`, an integer array [E,2], an int32 CUDA tensor, or
    `mesh_edges()`. `image_index`: as in `draw_landmarks`."""
    if image_index is not None:
        return _by_frame(draw_mesh, predictions, images, image_index, out, edges=edges)
    items, _ = _image_list(images)
    verts = _field(predictions, "projected_vertices", len(items), 2)
    return draw_segments(images, verts, edges, color=EDGE_COLOR, out=out)


# -- pose ---------------------------------------------------------------------------------------------------------------------------
def limit_angle(angle, pi=180.0):
    """model_training/model/flame.py:239-251, degrees."""
    if angle < -pi:
        k = -2 * (int(angle / pi) // 2)
        angle = angle + k * pi
    if angle > pi:
        k = 2 * ((int(angle / pi) + 1) // 2)
        angle = angle - k * pi
    return angle


def calculate_rpy(params_3dmm) -> List[RPY]:
    """model_training/model/flame.py:254-264 for every row of `params_3dmm` [B,413] (or [413]): `rot_mat_from_6dof` in float32,
    transposed, scipy's `Rotation.from_matrix(..).as_euler("xyz", degrees=True)`, then (roll, pitch, yaw) = limit_angle of
    (a[2], a[0] - 180, a[1]). On the host: the 24 bytes of rotation per image are copied from a device tensor, which SYNCHRONISES."""
    from scipy.spatial.transform import Rotation

    from .autograd import six_dof_to_matrix

    p = params_3dmm if isinstance(params_3dmm, Tensor) else torch.as_tensor(np.asarray(params_3dmm))
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2 or p.shape[1] != sum(FLAME_CONSTS.values()):
        raise ValueError(f"params_3dmm: expected [B,{sum(FLAME_CONSTS.values())}], got shape {tuple(p.shape)}")
    rotation = FlameParams.from_3dmm(p, FLAME_CONSTS).rotation.detach().float().cpu()
    out = []
    for row in rotation:  # one row at a time, as the reference's batch of one
        rot_mat = six_dof_to_matrix(row[None]).numpy()[0]
        angle = Rotation.from_matrix(np.transpose(rot_mat)).as_euler("xyz", degrees=True)
        out.append(RPY(*map(limit_angle, [angle[2], angle[0] - 180, angle[1]])))
    return out


_POSE_EDGES = np.array([[0, 1], [1, 4], [1, 5], [0, 2], [2, 6], [2, 7], [0, 3], [3, 8], [3, 9]], dtype=np.int32)
_POSE_SEGMENT_COLORS = np.repeat(np.array(POSE_COLORS, dtype=np.uint8), 3, axis=0)


def pose_thickness(h: int) -> int:
    t = int(h * 0.005)  # demo_utils.py:90
    if t < 1:
        raise ValueError(f"draw_pose: the arrows' thickness int({h} * 0.005) is 0 (cv2 rejects it too); the image needs 200 rows")
    return t


def pose_points(rpy: RPY, h: int, w: int) -> np.ndarray:
    """The ten points of the three arrows (demo_utils.py:73-92; cv2.arrowedLine's tips), int64 [10,2]: the centre, the three end
    points (`int()` truncation), and per arrow the two tip ends at 0.1 of its length, +- pi / 4, rounded half to even."""
    tdx, tdy = w // 2, h // 2
    roll, pitch, yaw = rpy.roll * np.pi / 180, rpy.pitch * np.pi / 180, -(rpy.yaw * np.pi / 180)
    size = h // 10
    x1 = size * (np.cos(yaw) * np.cos(roll)) + tdx
    y1 = size * (np.cos(pitch) * np.sin(roll) + np.cos(roll) * np.sin(pitch) * np.sin(yaw)) + tdy
    x2 = size * (-np.cos(yaw) * np.sin(roll)) + tdx
    y2 = size * (np.cos(pitch) * np.cos(roll) - np.sin(pitch) * np.sin(yaw) * np.sin(roll)) + tdy
    x3 = size * (np.sin(yaw)) + tdx
    y3 = size * (-np.cos(yaw) * np.sin(pitch)) + tdy
    centre = (int(tdx), int(tdy))
    ends = [(int(x1), int(y1)), (int(x2), int(y2)), (int(x3), int(y3))]
    tips = []
    for end in ends:
        tip = 0.1 * math.hypot(centre[0] - end[0], centre[1] - end[1])
        angle = math.atan2(centre[1] - end[1], centre[0] - end[0])
        for s in (1, -1):
            tips.append((round(end[0] + tip * math.cos(angle + s * math.pi / 4)), round(end[1] + tip * math.sin(angle + s * math.pi / 4))))
    return np.array([centre] + ends + tips, dtype=np.int64)


def draw_pose(predictions: Predictions, images: Images, out: Optional[Images] = None, image_index=None, angles: str = "host"):
    """demo_utils.py:68-94: the head's three axes as arrows from the image centre, colours (0,0,255), (0,255,0), (255,0,0) in
    that order, thickness `int(h * 0.005)` (ValueError where that is 0). An arrow is three solid segments: the shaft, then the two
    tips from its end point. The angles come from `calculate_rpy`, which synchronises; the segment ends are float64 on the host.
    `image_index`: as in `draw_landmarks`; every head's arrows start at the centre of its frame, as the reference draws them.
    `angles="device"`: the point table comes from `pose.head_pose` (`dad3d_head_pose`: the same route to the angles, in a kernel)
    and goes straight into the segment launch; no `calculate_rpy`, no wait. A row whose rotation is NaN / Inf or degenerate, on
    which `calculate_rpy` raises, then draws ten points at the centre instead."""
    if angles not in ("host", "device"):
        raise ValueError(f"angles: 'host' or 'device', got {angles!r}")
    if image_index is not None:
        return _by_frame(draw_pose, predictions, images, image_index, out, angles=angles)
    items, _ = _image_list(images)
    for t in items:
        pose_thickness(t.shape[0])
    if angles == "device":
        from .pose import head_pose

        params = _field(predictions, "3dmm_params", len(items), 1)
        if params.shape[1] != sum(FLAME_CONSTS.values()):
            raise ValueError(f"params_3dmm: expected [B,{sum(FLAME_CONSTS.values())}], got shape {tuple(params.shape)}")

        def device_tables_for(idx, h, w, device):
            rows = params if idx == list(range(params.shape[0])) else params[torch.as_tensor(idx, device=params.device)]
            return head_pose(rows.to(device), size=(h, w), want=("points",)).points

        def device_launch(src, dst, tab, h, w):
            _launch_segments(src, dst, tab, torch.from_numpy(_POSE_EDGES).to(src.device), torch.from_numpy(_POSE_SEGMENT_COLORS).to(src.device), 0,
                             pose_thickness(h))

        return _draw(images, out, device_tables_for, device_launch)
    rpy = calculate_rpy(_field(predictions, "3dmm_params", len(items), 1))

    def tables_for(idx, h, w, device):
        return torch.from_numpy(np.stack([pose_points(rpy[i], h, w) for i in idx]).astype(np.float32)).to(device)

    def launch(src, dst, tab, h, w):
        _launch_segments(src, dst, tab, torch.from_numpy(_POSE_EDGES).to(src.device), torch.from_numpy(_POSE_SEGMENT_COLORS).to(src.device), 0,
                         pose_thickness(h))

    return _draw(images, out, tables_for, launch)
