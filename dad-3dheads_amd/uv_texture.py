"""UV-texture bake (the reference demo's `uv_texture` output): a drop-in for `inference/uv_texture.py` `UVTextureCreator`.

Same surface as the reference (`get_mesh`, `_compute_texture_map`, `__call__`, the `texture_data` dict), plus the batched
device-resident entry `bake_batch`: ONE fused decode launch (`to_2d=False`, translation z := 0) followed by the float64 vertex
normals and the texel bake (csrc/uv_texture.hip); vertices, normals, photos and textures never leave HBM. For heads tracked in
a video: `bake_frames` (head k read from the frame its `image_index` names, csrc/uv_texture_frames.hip), `TextureAccumulator` (one
texture per tracker slot, the best view of every texel kept over time) and `render_frames` (the textured heads drawn into their frames).
`occlusion="self"` on the two former adds what the reference's rule lacks, a depth test of every sample against the head's own depth
map (`UVMap.depth_frames`, csrc/uv_texture_occlusion.hip); it is off by default.

What the reference computes, per candidate i of the atlas (`_compute_texture_map`, uv_texture.py:21-46), in float64:
    p = v[a] * b0 + v[b] * b1 + v[c] * b2,  the same with the vertex normals,  n_dot_view = -n.z
    (x, y) = np.round(p[:2]).astype(int)      (half to even)
    skip if n_dot_view < 0; write texture[y_coords[id], x_coords[id]] = image[y, x] if 0 < x < W and 0 < y < H
in candidate order (the last writer wins), zeros elsewhere. The GPU bake gives every texel its candidates in descending order
and takes the first that passes, which is the same texel.

Parity labels: the vertex normals are psbody-mesh's `Mesh.estimate_vertex_normals`, restated from its published source (psbody
is not installed: unpinned here); the faces are the packaged FLAME topology (`assets/flame_static.npz` `faces`), assumed equal
to `generic_model.pkl['f']`, which is absent; the atlas (`texture_data.npy`) is not redistributed: pass its path or set
`DAD3D_TEXTURE_DATA` (`synthetic.synthetic_texture_data` is a stand-in for tests and benchmarks only).

One difference from the reference: a candidate whose texel lies outside the texture is refused when the creator is built
(IndexError); the reference raises only when such a candidate passes both tests on some image.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .head_mesh import HeadMesh
from .Sim3DR.frames import DeviceFrames
from .Sim3DR.mesh import Mesh
from .synthetic import load_static


def load_texture_data(path: str) -> dict:
    """uv_texture.py:17: the atlas dict of `texture_data.npy`."""
    return np.load(path, allow_pickle=True, encoding="latin1").item()


def _resolve_texture_data(texture_data: Union[str, dict, None]) -> dict:
    if isinstance(texture_data, dict):
        return texture_data
    path = texture_data if texture_data is not None else os.environ.get("DAD3D_TEXTURE_DATA")
    if not path or not os.path.isfile(path):
        raise FileNotFoundError(
            "UV texture atlas not found. The reference ships without `inference/texture_data.npy`; pass texture_data=<path or "
            "dict> or set DAD3D_TEXTURE_DATA.")
    return load_texture_data(path)


def texel_table(texture_data: dict) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The candidate table the handle is built from, in candidate order: texel y * S + x (int32; `astype(int)` truncation,
    NumPy's negative indices wrapped), vertex ids int32 [n,3], barycentrics float64 [n,3], and S. IndexError for a texel
    outside the texture."""
    s = int(texture_data["img_size"])
    ids = np.asarray(texture_data["valid_pixel_ids"]).astype(np.int64)
    ty = np.asarray(texture_data["y_coords"])[ids].astype(int)
    tx = np.asarray(texture_data["x_coords"])[ids].astype(int)
    bad = (ty < -s) | (ty >= s) | (tx < -s) | (tx >= s)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise IndexError(f"texture_data candidate {i}: texel (y {int(ty[i])}, x {int(tx[i])}) is outside the {s} x {s} texture")
    texel = ((ty % s) * s + (tx % s)).astype(np.int32)
    verts = np.ascontiguousarray(np.asarray(texture_data["valid_pixel_3d_faces"]), dtype=np.int32).reshape(-1, 3)
    bary = np.ascontiguousarray(np.asarray(texture_data["valid_pixel_b_coords"]), dtype=np.float64).reshape(-1, 3)
    if not (len(texel) == len(verts) == len(bary)):
        raise ValueError(f"texture_data: {len(texel)} pixel ids, {len(verts)} vertex triples, {len(bary)} barycentric rows")
    return np.ascontiguousarray(texel), verts, bary, s


def texel_coords(vt: np.ndarray, size: int) -> np.ndarray:
    """Texture coordinates `vt [T,2]` in [0, 1] (u to the right, v UP: the OBJ convention) -> float32 texel units for an
    S x S texture: column u * (S - 1), row (1 - v) * (S - 1), so that (0, 1) is the centre of texel [0, 0] and (1, 0) the
    centre of texel [S-1, S-1]. This is the convention `synthetic.synthetic_texcoords` is written in; whether upstream's
    `texture_data.npy` follows it is unverified (the file is absent)."""
    vt = np.asarray(vt, dtype=np.float64)
    if vt.ndim != 2 or vt.shape[1] < 2:
        raise ValueError(f"vt must have shape [T, 2], got {vt.shape}")
    return np.stack([vt[:, 0] * (size - 1), (1.0 - vt[:, 1]) * (size - 1)], 1)


def _check_image(image) -> np.ndarray:
    # as strict as the Sim3DR wrapper: the bake reads 3-channel uint8 pixels and nothing else
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image must be a uint8 numpy array [H,W,3], got "
                         f"{getattr(image, 'dtype', type(image))} {getattr(image, 'shape', '')}")
    return np.ascontiguousarray(image)


class UVMap:
    """The device handle (dad3d_uvmap): a mesh's vertex -> face lists and an atlas' texel -> candidate table in HBM."""

    def __init__(self, faces: np.ndarray, n_verts: int, texture_data: dict, device: Optional[int] = None):
        self._lib = _lib.load()
        _lib.require_gpu()
        self.device = torch.cuda.current_device() if device is None else int(device)
        texel, verts, bary, s = texel_table(texture_data)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        handle = C.c_void_p()
        _lib.check(self._lib.dad3d_uvmap_create(f.ctypes.data, len(f), int(n_verts), texel.ctypes.data, verts.ctypes.data,
                                                bary.ctypes.data, len(texel), s, self.device, C.byref(handle)))
        self._handle = handle
        self._owner_pid = os.getpid()
        self.size = s
        self.n_verts = int(n_verts)

    def __del__(self):
        h = self.__dict__.get("_handle")
        self.__dict__["_handle"] = None
        if h and self.__dict__.get("_owner_pid") == os.getpid():  # a forked child does not own the device state (see FLAMELayer.__del__)
            try:
                self._lib.dad3d_uvmap_destroy(h)
            except Exception:
                pass

    def _check(self, t: Tensor, name: str, dtype, shape) -> None:
        if t.device != torch.device("cuda", self.device) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected a contiguous {dtype} tensor {shape} on cuda:{self.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def vertex_normals(self, vertices: Tensor, out: Optional[Tensor] = None) -> Tensor:
        b = vertices.shape[0]
        self._check(vertices, "vertices", torch.float32, (b, self.n_verts, 3))
        if out is None:
            out = torch.empty((b, self.n_verts, 3), dtype=torch.float64, device=vertices.device)
        self._check(out, "normals", torch.float64, (b, self.n_verts, 3))
        stream = torch.cuda.current_stream(vertices.device).cuda_stream
        _lib.check(self._lib.dad3d_uvmap_vertex_normals(self._handle, out.data_ptr(), vertices.data_ptr(), b, stream))
        return out

    def bake(self, vertices: Tensor, normals: Tensor, images: Tensor, hw: Optional[Tensor] = None,
             out: Optional[Tensor] = None) -> Tensor:
        b = vertices.shape[0]
        self._check(vertices, "vertices", torch.float32, (b, self.n_verts, 3))
        self._check(normals, "normals", torch.float64, (b, self.n_verts, 3))
        if images.ndim != 4 or images.shape[0] != b or images.shape[3] != 3:
            raise ValueError(f"images: expected [B={b},H,W,3], got {tuple(images.shape)}")
        _, h, w, _ = images.shape
        self._check(images, "images", torch.uint8, (b, h, w, 3))
        if hw is not None:
            self._check(hw, "hw", torch.int32, (b, 2))
        s = self.size
        if out is None:
            out = torch.empty((b, s, s, 3), dtype=torch.uint8, device=images.device)
        self._check(out, "out", torch.uint8, (b, s, s, 3))
        stream = torch.cuda.current_stream(images.device).cuda_stream
        _lib.check(self._lib.dad3d_uvmap_bake(self._handle, out.data_ptr(), vertices.data_ptr(), normals.data_ptr(),
                                              images.data_ptr(), hw.data_ptr() if hw is not None else None, b, h, w, stream))
        return out

    def _frames_and_index(self, frames, image_index, n: int):
        dev = torch.device("cuda", self.device)
        fr = frames if isinstance(frames, DeviceFrames) else DeviceFrames(frames, dev)
        if fr.device.device != dev:
            raise ValueError(f"frames: on {fr.device.device}, the map on {dev}")
        if isinstance(image_index, Tensor) and image_index.is_cuda:
            idx = image_index
        else:
            idx = torch.as_tensor(np.asarray(image_index, dtype=np.int32).reshape(-1)).to(dev)
        self._check(idx, "image_index", torch.int32, (n,))
        return fr, idx

    def depth_frames(self, vertices: Tensor, frames, image_index, depth_side: int = 512, out=None) -> Tuple[Tensor, Tensor, Tensor]:
        """Depth maps of heads in frames (`dad3d_uvmap_depth_frames`): for head k the nearest z of its own surface at every pixel of
        its box in `frames[image_index[k]]`. vertices `[N,V,3]` float32 in the bake's coordinates (frame pixel x, pixel y, z with the
        viewer at -z: the nearer surface has the SMALLER z); `frames` and `image_index` as in `bake_frames` (no pixel is read).
        -> (depth float32 `[N,D,D]`, window int32 `[N,4]` = {x0, y0, ww, wh}, flags int32 `[N]`), D = `depth_side` in 1..4096:
        `depth[k, j, i]` for `j < wh, i < ww` belongs to pixel `(x0 + i, y0 + j)`, `+inf` where no triangle covers it; entries outside
        the window are not written. Flags: `_lib.BAKE_FLAG_INDEX`, `BAKE_FLAG_NONFINITE` (a NaN or inf vertex), `BAKE_FLAG_DEPTH_WINDOW`
        (the box is larger than D); a flagged head has the window {0,0,0,0} and an untouched map. A head outside its frame has an
        empty window and no flag. `out`: a depth tensor, or the tuple (depth, window, flags), to write into. Three launches on the
        current stream, no host wait."""
        n = vertices.shape[0]
        d = int(depth_side)
        dev = torch.device("cuda", self.device)
        if not 1 <= d <= _lib.BAKE_MAX_DEPTH_SIDE:
            raise ValueError(f"depth_side: {depth_side} outside 1..{_lib.BAKE_MAX_DEPTH_SIDE}")
        self._check(vertices, "vertices", torch.float32, (n, self.n_verts, 3))
        fr, idx = self._frames_and_index(frames, image_index, n)
        depth, window, flags = out if isinstance(out, (tuple, list)) else (out, None, None)
        if depth is None:
            depth = torch.empty((n, d, d), dtype=torch.float32, device=dev)
        if window is None:
            window = torch.empty((n, 4), dtype=torch.int32, device=dev)
        if flags is None:
            flags = torch.empty(n, dtype=torch.int32, device=dev)
        self._check(depth, "depth", torch.float32, (n, d, d))
        self._check(window, "window", torch.int32, (n, 4))
        self._check(flags, "depth flags", torch.int32, (n,))
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._lib.dad3d_uvmap_depth_frames(self._handle, depth.data_ptr(), window.data_ptr(), vertices.data_ptr(),
                                                      fr.device.data_ptr(), fr.host.ctypes.data, len(fr), idx.data_ptr(), n, d,
                                                      flags.data_ptr(), stream))
        return depth, window, flags

    def bake_frames(self, vertices: Tensor, normals: Tensor, frames, image_index, out: Optional[Tensor] = None,
                    score: Optional[Tensor] = None, occlusion: Optional[str] = None, depth_side: int = 512, depth_bias: float = 1.0,
                    slope_bias: float = 1.0, depth=None) -> Tuple[Tensor, Tensor]:
        """The bake for heads that name their frames (`dad3d_uvmap_bake_frames`): head k reads `frames[image_index[k]]` and owns
        texture k. vertices `[N,V,3]` float32 in frame coordinates, normals `[N,V,3]` float64. `frames`: a list of uint8 CUDA
        tensors `[H,W,3]` of any sizes and row strides (views included), one `[B,H,W,3]` tensor, or a `DeviceFrames` (its table is
        uploaded once: what a graph capture needs). `image_index`: an int32 CUDA tensor `[N]`, used as it is and never read on the
        host, or a host sequence, uploaded. `score=None`: the plain bake into `out` (allocated when None), every byte written.
        `score [N,S,S]` float32: `out` (required) and `score` are the running state, a texel is replaced iff its new sample's
        n_dot_view is greater ("best view wins"). -> (textures uint8 `[N,S,S,3]`, int32 flags `[N]`: 0 or `_lib.BAKE_FLAG_INDEX`, the
        index names no frame). Async on the current stream, no host wait.

        `occlusion="self"`: `depth_frames` (into `depth` -- what its `out` takes -- or tensors allocated here) and then
        `dad3d_uvmap_bake_frames_occluded`: a candidate whose point lies behind the head's own surface at its pixel by more than
        `depth_bias + slope_bias * (|nx| + |ny|) / n_dot_view` pixels of depth is skipped and the texel's next candidate tried. The
        defaults 1.0 and 1.0 are untuned design choices. The flags then also carry `BAKE_FLAG_NONFINITE` and `BAKE_FLAG_DEPTH_WINDOW`
        (the head's box exceeds `depth_side`); a head with any flag gives zeros, or with `score` keeps its state. `occlusion=None`
        (the default) is the call without the depth test, untouched; the other keywords are then ignored."""
        if occlusion not in (None, "self"):
            raise ValueError(f"occlusion: {occlusion!r}, expected None or 'self'")
        if occlusion is not None and not (np.isfinite(depth_bias) and depth_bias >= 0 and np.isfinite(slope_bias) and slope_bias >= 0):
            raise ValueError(f"depth_bias {depth_bias} and slope_bias {slope_bias} must be finite and not negative")
        n = vertices.shape[0]
        dev = torch.device("cuda", self.device)
        self._check(vertices, "vertices", torch.float32, (n, self.n_verts, 3))
        self._check(normals, "normals", torch.float64, (n, self.n_verts, 3))
        fr, idx = self._frames_and_index(frames, image_index, n)
        s = self.size
        if score is not None:
            if out is None:
                raise ValueError("score: accumulation needs `out`, the textures the scores belong to")
            self._check(score, "score", torch.float32, (n, s, s))
        if out is None:
            out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=dev)
        self._check(out, "out", torch.uint8, (n, s, s, 3))
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if occlusion is None:
            _lib.check(self._lib.dad3d_uvmap_bake_frames(self._handle, out.data_ptr(), score.data_ptr() if score is not None else None,
                                                         vertices.data_ptr(), normals.data_ptr(), fr.device.data_ptr(), fr.host.ctypes.data,
                                                         len(fr), idx.data_ptr(), n, flags.data_ptr(), stream))
            return out, flags
        d_map, window, d_flags = self.depth_frames(vertices, fr, idx, depth_side=depth_side, out=depth)
        _lib.check(self._lib.dad3d_uvmap_bake_frames_occluded(
            self._handle, out.data_ptr(), score.data_ptr() if score is not None else None, vertices.data_ptr(), normals.data_ptr(),
            fr.device.data_ptr(), fr.host.ctypes.data, len(fr), idx.data_ptr(), n, d_map.data_ptr(), window.data_ptr(), d_flags.data_ptr(),
            int(depth_side), float(depth_bias), float(slope_bias), flags.data_ptr(), stream))
        return out, flags


class UVTextureCreator:
    """`UVTextureCreator(texture_data=path | dict | None, head_mesh=None, static=None, **head_mesh_kwargs)`.

    `texture_data` None reads the path in DAD3D_TEXTURE_DATA. `head_mesh_kwargs` go to `HeadMesh` (e.g. `flame_model`,
    `device`) when no `head_mesh` is given, as in `pncc.PNCCEstimator`."""

    def __init__(self, texture_data: Union[str, dict, None] = None, head_mesh: Optional[HeadMesh] = None,
                 static: Optional[dict] = None, tex_coords: Optional[np.ndarray] = None,
                 tex_triangles: Optional[np.ndarray] = None, **head_mesh_kwargs):
        self._tex_layout = None if tex_coords is None else (tex_coords, tex_triangles)
        self._renderer: Optional[Mesh] = None
        self.texture_data = _resolve_texture_data(texture_data)
        texel_table(self.texture_data)  # refuse an out-of-range texel before any device work
        st = static if static is not None else load_static()
        self.head_mesh = head_mesh if head_mesh is not None else HeadMesh(static=st, **head_mesh_kwargs)
        # generic_model.pkl is absent: its faces are taken to be the packaged FLAME topology
        self.flame_model = {"f": np.asarray(st["faces"]).astype(np.uint32)}
        self.img_size = int(self.texture_data["img_size"])
        self._maps: Dict[Tuple[int, bytes], UVMap] = {}
        self._normals: Optional[Tensor] = None

    # -- handles ------------------------------------------------------------------------------------------
    def _map(self, faces: np.ndarray, n_verts: int) -> UVMap:
        f = np.ascontiguousarray(faces, dtype=np.int32)
        key = (n_verts, f.tobytes())
        m = self._maps.get(key)
        if m is None:
            m = UVMap(f, n_verts, self.texture_data, device=self.head_mesh.flame.device_index)
            self._maps[key] = m
        return m

    @property
    def uv_map(self) -> UVMap:
        """The handle of the head mesh's topology (the one `bake_batch` uses), built on first use."""
        m = self.__dict__.get("_head_map")
        if m is None:
            m = self._map(self.flame_model["f"], int(self.head_mesh.flame.n_verts))
            self._head_map = m
        return m

    def reserve(self, batch: int) -> None:
        """Size the normals buffer of `bake_batch` for `batch` images, so that a later call can be captured in a graph."""
        m = self.uv_map
        if self._normals is None or self._normals.shape[0] < batch:
            self._normals = torch.empty((batch, m.n_verts, 3), dtype=torch.float64, device=self.head_mesh.flame.torch_device)

    # -- reference surface (single image, host arrays) ----------------------------------------------------
    def get_mesh(self, predicted_mesh: Dict[str, Tensor]) -> SimpleNamespace:
        """uv_texture.py:51-53: `Mesh(v, f)` with `v` float64 [V,3] (psbody's dtype) and `f` the faces. Sets translation z := 0
        in `predicted_mesh["3dmm_params"]`, like the reference."""
        with torch.no_grad():
            v = self.head_mesh.reprojected_vertices(params_3dmm=predicted_mesh["3dmm_params"], to_2d=False)[0]
        return SimpleNamespace(v=v.detach().cpu().numpy().astype(np.float64), f=self.flame_model["f"])

    def _compute_texture_map(self, source_img: np.ndarray, target_mesh) -> np.ndarray:
        """uv_texture.py:21-46 on the GPU -> uint8 [S,S,3]. `target_mesh.v` must hold float32 values (the decode's): the
        kernels read fp32 vertices and widen them exactly."""
        img = _check_image(source_img)
        v64 = np.asarray(target_mesh.v, dtype=np.float64)
        v32 = v64.astype(np.float32)
        if not np.array_equal(v32.astype(np.float64), v64, equal_nan=True):
            raise ValueError("target_mesh.v must hold float32 values (the GPU bake widens fp32 vertices to float64 exactly)")
        m = self._map(np.asarray(target_mesh.f), v64.shape[0])
        dev = torch.device("cuda", m.device)
        vert = torch.from_numpy(v32[None]).to(dev)
        normals = m.vertex_normals(vert)
        tex = m.bake(vert, normals, torch.from_numpy(img[None]).to(dev))
        return tex[0].cpu().numpy()

    def __call__(self, image: np.ndarray, mesh: Dict[str, Tensor], *args, **kwargs) -> np.ndarray:
        return self._compute_texture_map(image, self.get_mesh(mesh))

    # -- MI355X-native batched entries ---------------------------------------------------------------------
    def vertex_normals(self, vertices: Tensor) -> Tensor:
        """`vertices [B,V,3]` fp32 on the GPU -> psbody's vertex normals `[B,V,3]` float64 (see the module docstring)."""
        return self.uv_map.vertex_normals(vertices)

    def bake_batch(self, params: Tensor, images: Tensor, hw: Optional[Tensor] = None, mutate: bool = True,
                   out: Optional[Tensor] = None) -> Tensor:
        """`params [B,413]` fp32 and `images [B,H,W,3]` uint8 on the GPU -> UV textures `[B,S,S,3]` uint8 on the GPU.

        Three launches on the current stream, no host sync: the fused decode (`proj=True, to_2d=False`; `mutate` writes
        translation z := 0 into `params` like `HeadMesh.reprojected_vertices`), the float64 normals and the bake. `hw [B,2]`
        int32: each photo's own (height, width) inside a padded batch. Capturable in a graph after one call of the same
        batch size or after `reserve(batch)`. Composes with the predictor:

            params = FaceMeshPredictor(...).predict_tensor(images)["3dmm_params"]   # [B,413] on the GPU
            textures = creator.bake_batch(params, photos)                          # photos [B,H,W,3] uint8 on the GPU
        """
        m = self.uv_map
        b = params.shape[0]
        self.reserve(b)
        verts = self.head_mesh.flame.decode(params, proj=True, to_2d=False, mutate=mutate)["proj"]
        normals = m.vertex_normals(verts, out=self._normals[:b])
        return m.bake(verts, normals, images, hw=hw, out=out)

    def bake_frames(self, params: Tensor, frames, image_index, mutate: bool = True, out: Optional[Tensor] = None,
                    score: Optional[Tensor] = None, occlusion: Optional[str] = None, depth_side: int = 512, depth_bias: float = 1.0,
                    slope_bias: float = 1.0, depth=None) -> Tuple[Tensor, Tensor]:
        """`params [N,413]` fp32 on the GPU, in FRAME coordinates (what `predict_boxes` / `HeadTracker.step` return), head k read from
        `frames[image_index[k]]` -> (textures `[N,S,S,3]` uint8, flags `[N]` int32), both on the GPU.

        Three launches on the current stream, no host sync: the decode of `bake_batch` (`proj=True, to_2d=False`, no flip; `mutate`
        writes translation z := 0 into `params`), the float64 normals and `UVMap.bake_frames` -- see there for `frames`, `image_index`,
        `out`, `score`, the flags and `occlusion="self"` with its keywords (three more launches: the head's own depth map, then the bake
        with the depth test). A lost slot of the tracker (`image_index == -1`) is flagged and, with `score`, changes nothing.
        Capturable in a graph after one call of the same N or after `reserve(N)`, with `frames` a `DeviceFrames`."""
        m = self.uv_map
        n = params.shape[0]
        self.reserve(n)
        verts = self.head_mesh.flame.decode(params, proj=True, to_2d=False, mutate=mutate)["proj"]
        normals = m.vertex_normals(verts, out=self._normals[:n])
        return m.bake_frames(verts, normals, frames, image_index, out=out, score=score, occlusion=occlusion, depth_side=depth_side,
                             depth_bias=depth_bias, slope_bias=slope_bias, depth=depth)

    # -- textured render: the other half of the bake -------------------------------------------------------
    def set_texcoords(self, tex_coords: np.ndarray, tex_triangles: np.ndarray) -> None:
        """The corner layout `render_batch` samples with: `tex_coords [T,2]` in TEXEL units of the S x S texture (x = column,
        y = row) and `tex_triangles [F,3]`, one row per face of the head topology, a negative row for a face without texture
        coordinates (left out of the render). Replaces what the atlas' `vt` / `ft` keys or the constructor gave."""
        self._tex_layout = (tex_coords, tex_triangles)
        self._renderer = None

    @property
    def renderer(self) -> Mesh:
        """The `Sim3DR.Mesh` of the faces that have texture coordinates, with those attached; built on first use.

        The layout comes from `set_texcoords` / the constructor's `tex_coords`, `tex_triangles`, else from the atlas' keys
        `vt` [T,2] and `ft` [F,3] through `texel_coords` (upstream's `texture_data.npy` is believed to carry them: unverified,
        the file is absent; `synthetic.synthetic_texcoords` supplies them for the synthetic atlas)."""
        if self._renderer is None:
            if self._tex_layout is not None:
                tc, ft = self._tex_layout
            elif "vt" in self.texture_data and "ft" in self.texture_data:
                tc, ft = texel_coords(self.texture_data["vt"], self.img_size), self.texture_data["ft"]
            else:
                raise ValueError("render_batch needs texture coordinates: texture_data has no 'vt' / 'ft' keys; pass tex_coords and "
                                 "tex_triangles (texel units) to the constructor or to set_texcoords")
            faces = np.asarray(self.flame_model["f"]).astype(np.int32)
            ft = np.asarray(ft).astype(np.int64)
            if ft.shape != faces.shape:
                raise ValueError(f"tex_triangles: expected one row per face {faces.shape}, got {ft.shape}")
            keep = (ft >= 0).all(1)
            mesh = Mesh(np.ascontiguousarray(faces[keep]), int(self.head_mesh.flame.n_verts), device=self.head_mesh.flame.device_index)
            mesh.set_texcoords(np.ascontiguousarray(np.asarray(tc)[:, :2], dtype=np.float32), np.ascontiguousarray(ft[keep], dtype=np.int32))
            self._renderer = mesh
        return self._renderer

    def reserve_render(self, batch: int, size: Optional[Tuple[int, int]] = None) -> None:
        """Size the raster scratch of `render_batch` for `batch` images of `size` (one throw-away render of a collapsed mesh),
        so that a later call of that shape allocates nothing and can be captured in a graph."""
        mesh = self.renderer
        h, w = size if size is not None else (self.head_mesh._image_size,) * 2
        dev = mesh.torch_device
        mesh.render_texture(torch.zeros((batch, mesh.nver, 3), dtype=torch.float32, device=dev),
                            torch.zeros((1, 1, 3), dtype=torch.uint8, device=dev),
                            torch.zeros((batch, h, w, 3), dtype=torch.uint8, device=dev))

    def render_batch(self, params: Tensor, textures: Tensor, bg: Optional[Tensor] = None, size: Optional[Tuple[int, int]] = None,
                     mapping: str = "bilinear", out: Optional[Tensor] = None, mutate: bool = True) -> Tensor:
        """`params [B,413]` fp32 and `textures` (what `bake_batch` returns: `[B,S,S,3]` uint8, or one shared `[S,S,3]`; float32
        works too) on the GPU -> the textured heads `[B,H,W,3]` on the GPU: the head re-rendered at the pose of `params`.

        One fused decode launch (`proj=True, to_2d=False`, z flipped as `PNCCEstimator.render_batch` does, because Sim3DR keeps
        the LARGER depth), then the geometry and tile launches of `Mesh.render_texture` (`_render_texture_core`,
        rasterize_kernel.cpp:358-463). The image is `out` when given (`bg` is copied into it first, without `bg` its own content is the
        background), else `bg` itself (rendered into, like `PNCCEstimator.render_batch`), else black uint8 of `size=(H, W)` (the head mesh's image size by default). No host sync; capturable in a graph after one call
        of the same shape or after `reserve_render(batch, size)`, with `out` given."""
        mesh = self.renderer
        b = params.shape[0]
        if out is None:
            if bg is not None:
                out = bg
            else:
                h, w = size if size is not None else (self.head_mesh._image_size,) * 2
                out = torch.zeros((b, h, w, 3), dtype=torch.uint8, device=mesh.torch_device)
        elif bg is not None:
            out.copy_(bg)
        verts = self.head_mesh.flame.decode(params, proj=True, to_2d=False, flip_z=True, mutate=mutate)["proj"]
        return mesh.render_texture(verts, textures, out, mapping=mapping)

    def render_frames(self, params: Tensor, textures, frames, image_index, mapping: str = "bilinear", mutate: bool = True) -> Tensor:
        """`params [N,413]` fp32 on the GPU in frame coordinates and `textures` (`[N,S,S,3]`, one shared `[S,S,3]`, uint8 or float32,
        or a `TextureAccumulator`) -> head k drawn with its texture into `frames[image_index[k]]`, in place: the decode of
        `render_batch` (z flipped), then `Mesh.render_texture_frames`. A later head of a frame paints over an earlier one.
        -> int32 CUDA flags `[N]` (`Mesh.rasterize_frames`). No host sync."""
        tex = textures.textures if isinstance(textures, TextureAccumulator) else textures
        if tex.ndim == 4 and tex.shape[0] > params.shape[0]:
            tex = tex[:params.shape[0]]  # fewer heads than slots: head k still samples texture k
        verts = self.head_mesh.flame.decode(params, proj=True, to_2d=False, flip_z=True, mutate=mutate)["proj"]
        return self.renderer.render_texture_frames(frames, verts, tex, image_index, mapping=mapping)


class TextureAccumulator:
    """The texture of every tracker slot, accumulated over the frames of a video, on the device: `textures` uint8 `[n,S,S,3]` and
    `score` float32 `[n,S,S]`, the n_dot_view of the sample each texel holds (-1: none yet).

    A one-frame bake is half empty, because the reference skips every texel whose normal faces away; over a video the head turns and
    `add` keeps, per texel, the sample seen most frontally ("best view wins": strictly greater n_dot_view replaces, a tie keeps the
    older sample). Head k of a call always goes to slot k -- the tracker's slots are fixed.

    `occlusion="self"`: every `add` first draws each head's own depth map (`UVMap.depth_frames`, `depth_side` pixels square, owned
    here) and skips the samples that lie behind it (`UVMap.bake_frames`: `depth_bias`, `slope_bias`, untuned defaults) -- without it
    a sample taken through the nose stays until a better-scored view arrives, which for a texel only ever seen at a grazing angle is
    never. Off by default. Not done: blending of samples, occlusion of a head by another head or an object (depths of different heads
    do not compare), temporal filtering."""

    def __init__(self, creator: UVTextureCreator, n_slots: int, occlusion: Optional[str] = None, depth_side: int = 512,
                 depth_bias: float = 1.0, slope_bias: float = 1.0):
        if int(n_slots) < 1:
            raise ValueError(f"n_slots: {n_slots}, at least 1")
        if occlusion not in (None, "self"):
            raise ValueError(f"occlusion: {occlusion!r}, expected None or 'self'")
        if not 1 <= int(depth_side) <= _lib.BAKE_MAX_DEPTH_SIDE:
            raise ValueError(f"depth_side: {depth_side} outside 1..{_lib.BAKE_MAX_DEPTH_SIDE}")
        self.occlusion, self.depth_side, self.depth_bias, self.slope_bias = occlusion, int(depth_side), float(depth_bias), float(slope_bias)
        self._depth = None  # (depth [n,D,D], window [n,4], flags [n]) with occlusion="self"
        self.creator = creator
        self.n_slots = int(n_slots)
        dev = creator.head_mesh.flame.torch_device
        s = creator.img_size
        self.textures = torch.zeros((self.n_slots, s, s, 3), dtype=torch.uint8, device=dev)
        self.score = torch.full((self.n_slots, s, s), -1.0, dtype=torch.float32, device=dev)
        self.reserve(self.n_slots)

    def reserve(self, n: int) -> None:
        """Size the creator's buffers, and with `occlusion="self"` the depth maps, windows and depth flags, for `n` heads a call, so
        that a later `add` can be captured in a graph."""
        n = int(n)
        self.creator.reserve(n)
        if self.occlusion is not None and (self._depth is None or self._depth[0].shape[0] < n):
            dev, d = self.textures.device, self.depth_side
            self._depth = (torch.empty((n, d, d), dtype=torch.float32, device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev),
                           torch.zeros(n, dtype=torch.int32, device=dev))

    def reset(self, slots=None, mask=None) -> None:
        """Zeros and score -1 for all slots (None) or the given ones (a sequence or an int64 CUDA tensor): what a caller does beside
        `HeadTracker.reseed`. `mask` instead of `slots`: an integer or bool tensor `[k]`, k <= n_slots, on the device; slot i < k is
        reset where the mask is not 0 (what `HeadTracker.update` does with the slots it spawned): masked fills, no index list. No
        host read."""
        if mask is not None:
            dev = self.textures.device
            if slots is not None:
                raise ValueError("reset: slots or mask, not both")
            if not isinstance(mask, Tensor) or mask.device != dev or mask.ndim != 1 or mask.shape[0] > self.n_slots or mask.is_floating_point():
                raise ValueError(f"mask: expected an integer or bool tensor [k <= {self.n_slots}] on {dev}")
            k, on = mask.shape[0], mask != 0
            self.textures[:k].masked_fill_(on.view(k, 1, 1, 1), 0)
            self.score[:k].masked_fill_(on.view(k, 1, 1), -1.0)
            return
        if slots is None:
            self.textures.zero_()
            self.score.fill_(-1.0)
            return
        idx = slots.to(self.textures.device, torch.int64) if isinstance(slots, Tensor) else torch.as_tensor(
            np.asarray(slots, dtype=np.int64).reshape(-1)).to(self.textures.device)
        self.textures.index_fill_(0, idx, 0)
        self.score.index_fill_(0, idx, -1.0)

    def add(self, predictions_or_params, frames, image_index=None) -> Tensor:
        """One frame set of the video: `predictions_or_params` the list of per-head dicts of `predict_boxes` / `HeadTracker.step`
        (their `3dmm_params` are stacked and `image_index=None` means their own, as `overlay.draw_heads` does) or a `[N,413]` tensor
        with `image_index`; N <= n_slots, head k into slot k. -> int32 CUDA flags `[N]` (`_lib.BAKE_FLAG_INDEX`: the slot named no
        frame and kept its state; with `occlusion="self"` also `BAKE_FLAG_NONFINITE` and `BAKE_FLAG_DEPTH_WINDOW`, likewise kept). Nothing waits for the device; the params are not mutated."""
        dev = self.textures.device
        if isinstance(predictions_or_params, Tensor):
            if image_index is None:
                raise ValueError("image_index: required with a params tensor")
            params, index = predictions_or_params, image_index
        else:
            from .overlay import _field, _head_index
            dicts = list(predictions_or_params)
            params = _field(dicts, "3dmm_params", len(dicts), 1).to(dev, torch.float32).contiguous()
            index = _head_index(dicts, image_index, dev)
        n = params.shape[0]
        if n > self.n_slots:
            raise ValueError(f"{n} heads for {self.n_slots} slots")
        if len(index) != n:
            raise ValueError(f"image_index: {len(index)} entries for {n} heads")
        if self.occlusion is None:
            _, flags = self.creator.bake_frames(params, frames, index, mutate=False, out=self.textures[:n], score=self.score[:n])
            return flags
        self.reserve(n)
        _, flags = self.creator.bake_frames(params, frames, index, mutate=False, out=self.textures[:n], score=self.score[:n],
                                            occlusion=self.occlusion, depth_side=self.depth_side, depth_bias=self.depth_bias,
                                            slope_bias=self.slope_bias, depth=tuple(t[:n] for t in self._depth))
        return flags

    def filled(self) -> Tensor:
        """bool `[n,S,S]` on the device: the texels that hold a sample."""
        return self.score > -1.0
