"""Batched, device-resident Sim3DR: torch CUDA tensors in, torch CUDA tensors out, async on the current stream.

One `Mesh` = one static triangle list (uploaded once together with its vertex->face incidence list).
All methods take a leading batch dimension; nothing is copied to the host.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _lib
from .frames import DeviceFrames


def _chk(t: Tensor, dtype, ndim: int, name: str, dev: torch.device) -> Tensor:
    if t.dtype != dtype or t.ndim != ndim or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor with {ndim} dims on {dev}, "
                         f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


class Mesh:
    def _verts(self, vertices: Tensor, name: str = "vertices") -> Tensor:
        """[B, nver, 3] float32 on this mesh's device -- the kernels index every vertex the triangle list names."""
        v = _chk(vertices, torch.float32, 3, name, self.torch_device)
        if tuple(v.shape[1:]) != (self.nver, 3):
            raise ValueError(f"{name}: expected [B, {self.nver}, 3], got {tuple(v.shape)}")
        return v

    def __init__(self, triangles, nver: int, device: Optional[int] = None):
        tri = np.ascontiguousarray(np.asarray(triangles))
        if tri.dtype != np.int32:
            raise ValueError(f"Buffer dtype mismatch, expected 'int' but got '{tri.dtype}'")  # rasterize.pyx typed buffer
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError("triangles must have shape [ntri, 3]")
        self._lib = _lib.load()
        _lib.require_gpu()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.ntri, self.nver = int(tri.shape[0]), int(nver)
        self._triangles = tri  # host copy: the default tex_triangles of set_texcoords
        self.has_texcoords = False
        h = C.c_void_p()
        _lib.check(self._lib.dad3d_mesh_create(tri.ctypes.data, self.ntri, self.nver, self.device_index, C.byref(h)))
        self._handle = h
        self._owner_pid = os.getpid()

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h and getattr(self, "_owner_pid", None) == os.getpid():  # a forked child does not own the device state (see FLAMELayer.__del__)
            try:
                self._lib.dad3d_mesh_destroy(h)
            except Exception:
                pass

    @property
    def torch_device(self) -> torch.device:
        return torch.device("cuda", self.device_index)

    def _stream(self):
        return torch.cuda.current_stream(self.torch_device).cuda_stream

    # -- normals -----------------------------------------------------------------------------------
    def normal_plan(self, batch: int = 1, entry: str = "get_normal", h: int = 0, w: int = 0) -> dict:
        """Which kernel a launch would take, from the launchers' own decision functions; nothing is launched.
        entry "get_normal" | "phong_light" (normals=None) | "render" (on h x w images; the batch plays no part).
        -> {"form": "table" | "lds" | "global" | "refused", "chunks": workgroups per image computing normals,
            "built": the table chunkings `dad3d_mesh_create` built, a subset of (1, 2, 4, 8)}"""
        entries = {"get_normal": _lib.PLAN_GET_NORMAL, "phong_light": _lib.PLAN_PHONG, "render": _lib.PLAN_RENDER}
        if entry not in entries:
            raise ValueError(f"entry: one of {sorted(entries)}, got {entry!r}")
        form, chunks, built = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.dad3d_mesh_normal_plan(self._handle, entries[entry], int(batch), int(h), int(w), C.byref(form),
                                                    C.byref(chunks), C.byref(built)))
        names = {_lib.FORM_REFUSED: "refused", _lib.FORM_TABLE: "table", _lib.FORM_LDS: "lds", _lib.FORM_GLOBAL: "global"}
        return {"form": names[form.value], "chunks": chunks.value, "built": tuple(1 << k for k in range(4) if built.value >> k & 1)}

    def get_normal(self, vertices: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
        """`_get_normal` per image: vertices [B,nver,3] -> unit vertex normals [B,nver,3]."""
        v = self._verts(vertices)
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs `out`")
            out = torch.empty_like(v)
        self._verts(out, "out")
        if out.shape[0] != v.shape[0]:
            raise ValueError("out: batch mismatch")
        _lib.check(self._lib.dad3d_mesh_get_normal(self._handle, out.data_ptr(), v.data_ptr(), v.shape[0],
                                                   _lib.NORMAL_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def get_tri_normal(self, vertices: Tensor, norm_flg: bool = False) -> Tensor:
        v = self._verts(vertices)
        out = torch.empty((v.shape[0], self.ntri, 3), dtype=torch.float32, device=v.device)
        _lib.check(self._lib.dad3d_mesh_get_tri_normal(self._handle, out.data_ptr(), v.data_ptr(), v.shape[0], int(norm_flg), self._stream()))
        return out

    def get_ver_normal(self, tri_normal: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
        t = _chk(tri_normal, torch.float32, 3, "tri_normal", self.torch_device)
        if tuple(t.shape[1:]) != (self.ntri, 3):
            raise ValueError(f"tri_normal: expected [B, {self.ntri}, 3], got {tuple(t.shape)}")
        if out is not None and (self._verts(out, "out").shape[0] != t.shape[0]):
            raise ValueError("out: batch mismatch")
        if out is None:
            out = torch.empty((t.shape[0], self.nver, 3), dtype=torch.float32, device=t.device)
        _lib.check(self._lib.dad3d_mesh_get_ver_normal(self._handle, out.data_ptr(), t.data_ptr(), t.shape[0],
                                                       _lib.NORMAL_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    # -- raster ------------------------------------------------------------------------------------
    def rasterize(self, vertices: Tensor, colors: Tensor, bg: Tensor, depth: Optional[Tensor] = None,
                  reverse: bool = False, alpha: float = 1.0) -> Tensor:
        """`_rasterize` per image, in place on `bg` [B,h,w,c] uint8 (returned). colors [B,nver,c] in [0,1]."""
        v = _chk(vertices, torch.float32, 3, "vertices", self.torch_device)
        img = _chk(bg, torch.uint8, 4, "bg", self.torch_device)
        col = _chk(colors, torch.float32, 3, "colors", self.torch_device)
        b, h, w, c = img.shape
        if col.shape != (b, self.nver, c) or v.shape != (b, self.nver, 3):
            raise ValueError("vertices/colors/bg batch or channel mismatch")
        dptr = None
        if depth is not None:
            dptr = _chk(depth, torch.float32, 3, "depth", self.torch_device).data_ptr()
        _lib.check(self._lib.dad3d_mesh_rasterize(self._handle, img.data_ptr(), v.data_ptr(), col.data_ptr(), dptr,
                                                  b, h, w, c, float(alpha), int(reverse), self._stream()))
        return img

    # -- heads into frames --------------------------------------------------------------------------
    def _frames_args(self, frames, vertices: Tensor, image_index):
        v = self._verts(vertices)
        dev = self.torch_device
        fr = frames if isinstance(frames, DeviceFrames) else DeviceFrames(frames, dev)
        if fr.device.device != dev:
            raise ValueError(f"frames: on {fr.device.device}, the mesh on {dev}")
        if isinstance(image_index, Tensor) and image_index.is_cuda:
            idx = _chk(image_index, torch.int32, 1, "image_index", dev)  # used as it is: never read on the host
        else:
            idx = torch.as_tensor(np.asarray(image_index, dtype=np.int32).reshape(-1)).to(dev)
        if idx.shape[0] != v.shape[0]:
            raise ValueError(f"image_index: {idx.shape[0]} entries for {v.shape[0]} heads")
        if v.shape[0] > _lib.FRAME_MAX_COUNT:
            raise ValueError(f"vertices: {v.shape[0]} heads, at most {_lib.FRAME_MAX_COUNT}")
        # without frames the C entries have nothing to do and write no flags: every index is outside [0, 0)
        flags = torch.empty(v.shape[0], dtype=torch.int32, device=dev) if len(fr) else torch.full((v.shape[0],), _lib.FRAME_FLAG_INDEX,
                                                                                                   dtype=torch.int32, device=dev)
        return fr, v, idx, flags

    def rasterize_frames(self, frames, vertices: Tensor, colors: Tensor, image_index, reverse: bool = False) -> Tensor:
        """Head k drawn into `frames[image_index[k]]`, for all heads of the call in one chain of launches: per frame what
        `Sim3DR.rasterize(vertices[k], triangles, colors[k], bg=frame)` gives when called for the frame's heads in ascending k --
        every head with a z-buffer of its own, so a later head paints over an earlier one wherever it covers.

        frames: a list of uint8 CUDA tensors `[H,W,3]` of any sizes and row strides (views included), one `[B,H,W,3]` tensor, or a
        `DeviceFrames` built from either (its table is uploaded once: what a graph capture needs); written in place. vertices,
        colors `[N,nver,3]` float32 (frame pixel x, pixel y, depth; colours in [0,1]). image_index: an int32 CUDA tensor `[N]`, used
        as it is, or a host sequence, uploaded. -> int32 CUDA `flags [N]`: 0 drawn, `_lib.FRAME_FLAG_INDEX` no such frame,
        `_lib.FRAME_FLAG_CAPACITY` the head did not fit the list pool of 4 * ntri * N entries (it holds every call whose on-screen
        triangle boxes are at most 64 x 64 pixels); a flagged head changes no byte. Async on the current stream, no host wait."""
        fr, v, idx, flags = self._frames_args(frames, vertices, image_index)
        col = self._verts(colors, "colors")
        if col.shape[0] != v.shape[0]:
            raise ValueError("colors: batch mismatch")
        _lib.check(self._lib.dad3d_mesh_rasterize_frames(self._handle, fr.device.data_ptr(), fr.host.ctypes.data, len(fr), v.data_ptr(),
                                                         col.data_ptr(), idx.data_ptr(), v.shape[0], int(bool(reverse)), flags.data_ptr(),
                                                         self._stream()))
        return flags

    def render_frames(self, frames, vertices: Tensor, image_index, reverse: bool = False, light_out: Optional[Tensor] = None,
                      ambient: float = 0.3, directional: float = 0.6, specular: float = 0.1, specular_exp: float = 5,
                      color_ambient: Sequence[float] = (1, 1, 1), color_directional: Sequence[float] = (1, 1, 1),
                      light_pos: Sequence[float] = (0, 0, 5), view_pos: Sequence[float] = (0, 0, 5)) -> Tensor:
        """`rasterize_frames` with RenderPipeline's light (lighting.py:37-71, texture=None) as the colours: the light of every head
        as `phong_light(vertices, None)` computes it (into `light_out`, allocated when None), then the frames chain. -> flags."""
        fr, v, idx, flags = self._frames_args(frames, vertices, image_index)
        light = torch.empty_like(v) if light_out is None else self._verts(light_out, "light_out")
        if light.shape[0] != v.shape[0]:
            raise ValueError("light_out: batch mismatch")
        cfg = _lib.LightC(float(ambient), float(directional), float(specular), float(specular_exp),
                          (C.c_float * 3)(*color_ambient), (C.c_float * 3)(*color_directional),
                          (C.c_float * 3)(*light_pos), (C.c_float * 3)(*view_pos))
        _lib.check(self._lib.dad3d_mesh_render_frames(self._handle, fr.device.data_ptr(), fr.host.ctypes.data, len(fr), v.data_ptr(),
                                                      light.data_ptr(), idx.data_ptr(), v.shape[0], C.byref(cfg),
                                                      _lib.RENDER_REVERSE if reverse else 0, flags.data_ptr(), self._stream()))
        return flags

    def frames_scratch_bytes(self) -> int:
        """Bytes of device scratch the handle holds for the frames chain (0 before the first call); it only ever grows."""
        n = C.c_size_t()
        _lib.check(self._lib.dad3d_mesh_frames_scratch_bytes(self._handle, C.byref(n)))
        return int(n.value)

    def rasterize_triangles(self, vertices: Tensor, h: int, w: int, depth: Optional[Tensor] = None):
        v = self._verts(vertices)
        b = v.shape[0]
        if depth is None:
            depth = torch.full((b, h, w), -1e8, dtype=torch.float32, device=v.device)
        tri_buf = torch.full((b, h, w), -1, dtype=torch.int32, device=v.device)
        bary = torch.zeros((b, h, w, 3), dtype=torch.float32, device=v.device)
        _lib.check(self._lib.dad3d_mesh_rasterize_triangles(self._handle, v.data_ptr(), depth.data_ptr(), tri_buf.data_ptr(),
                                                            bary.data_ptr(), b, h, w, self._stream()))
        return depth, tri_buf, bary

    # -- textured render ---------------------------------------------------------------------------
    def set_texcoords(self, tex_coords, tex_triangles=None) -> "Mesh":
        """Attach the (static) texture coordinates of `render_texture`: `tex_coords [T,2]` or `[T,3]` float32 in texel
        units (x = column, y = row; a third column is ignored) and `tex_triangles [ntri,3]` int32 indices into them
        (`None`: the mesh's own triangles, for one coordinate per vertex). Host arrays, uploaded once; returns self."""
        tc = np.ascontiguousarray(np.asarray(tex_coords))
        if tc.dtype != np.float32:
            raise ValueError(f"Buffer dtype mismatch, expected 'float' but got '{tc.dtype}'")
        if tc.ndim != 2 or tc.shape[1] not in (2, 3):
            raise ValueError(f"tex_coords must have shape [T, 2] or [T, 3], got {tc.shape}")
        if tex_triangles is None:
            if self._triangles is None:
                raise ValueError("tex_triangles: required for this mesh")
            tt = self._triangles
        else:
            tt = np.ascontiguousarray(np.asarray(tex_triangles))
        if tt.dtype != np.int32:
            raise ValueError(f"Buffer dtype mismatch, expected 'int' but got '{tt.dtype}'")
        if tt.shape != (self.ntri, 3):
            raise ValueError(f"tex_triangles must have shape [{self.ntri}, 3], got {tt.shape}")
        _lib.check(self._lib.dad3d_mesh_set_texcoords(self._handle, tc.ctypes.data, tc.shape[0], tc.shape[1], tt.ctypes.data))
        self.has_texcoords = True
        return self

    def render_texture(self, vertices: Tensor, texture: Tensor, out_or_bg: Tensor, depth: Optional[Tensor] = None,
                       mapping: str = "bilinear", indexing: str = "corner") -> Tensor:
        """`_render_texture_core` (rasterize_kernel.cpp:358-463) per image, in place on `out_or_bg` (returned): the mesh
        drawn with a texture sampled at the interpolated texture coordinates of `set_texcoords`.

        vertices [B,nver,3] float32; texture [B,th,tw,tc] or one shared [th,tw,tc], float32 or uint8; out_or_bg [B,h,w,c]
        float32 (bit-exact with the reference) or uint8 (the float result through `(unsigned char)`), 1 <= c <= min(4, tc),
        written where the mesh is drawn and kept elsewhere; depth [B,h,w] float32 in/out or None (start from -1e8).
        mapping "bilinear" | "nearest". indexing "corner" (x and y through `tex_triangles`) or "reference" (the C++
        function's own indexing: y through the mesh triangle). Pixels in the two-pixel border band of the image take any
        triangle whose bounding box reaches them, as in the reference. Async on the current stream, no host copy."""
        v = self._verts(vertices)
        if mapping not in ("bilinear", "nearest"):
            raise ValueError(f"mapping: 'bilinear' or 'nearest', got {mapping!r}")
        if indexing not in ("corner", "reference"):
            raise ValueError(f"indexing: 'corner' or 'reference', got {indexing!r}")
        dtypes = {torch.float32: _lib.DTYPE_F32, torch.uint8: _lib.DTYPE_U8}
        img, tex = out_or_bg, texture
        for t, name, dims in ((img, "out_or_bg", (4,)), (tex, "texture", (3, 4))):
            if t.dtype not in dtypes or t.ndim not in dims or not t.is_contiguous() or t.device != self.torch_device:
                raise ValueError(f"{name}: expected a contiguous float32 or uint8 tensor with {' or '.join(map(str, dims))} dims on "
                                 f"{self.torch_device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        b, h, w, c = img.shape
        if v.shape[0] != b or (tex.ndim == 4 and tex.shape[0] != b):
            raise ValueError("vertices/texture/out_or_bg batch mismatch")
        th, tw, tc = tex.shape[-3:]
        dptr = None
        if depth is not None:
            if tuple(depth.shape) != (b, h, w):
                raise ValueError("depth: expected [B, h, w] like out_or_bg")
            dptr = _chk(depth, torch.float32, 3, "depth", self.torch_device).data_ptr()
        _lib.check(self._lib.dad3d_mesh_render_texture(
            self._handle, img.data_ptr(), dtypes[img.dtype], v.data_ptr(), tex.data_ptr(), dtypes[tex.dtype], int(tex.ndim == 4), dptr,
            b, h, w, c, th, tw, tc, 0 if mapping == "nearest" else 1,
            _lib.TEX_INDEX_REFERENCE if indexing == "reference" else _lib.TEX_INDEX_CORNER, self._stream()))
        return img

    def render_texture_frames(self, frames, vertices: Tensor, textures: Tensor, image_index, mapping: str = "bilinear",
                              indexing: str = "corner") -> Tensor:
        """Textured heads through the frames chain: per frame, in ascending head order, `frame = (unsigned char)
        _render_texture_core(image=float(frame), vertices[k], .., textures[k], a fresh depth buffer at -1e8)` -- a later head paints
        over an earlier one wherever it covers a pixel, an uncovered pixel is not written.

        frames, vertices, image_index and the returned flags as for `rasterize_frames`. textures `[N,th,tw,tc]` (head k samples
        texture k) or one shared `[th,tw,tc]`, float32 or uint8, tc >= 3 (the first three channels are used). mapping "bilinear" |
        "nearest", indexing "corner" | "reference" as for `render_texture`. The two-pixel border band of `render_texture` is taken on
        each frame's own size (reference behaviour, kept; it only matters for a head whose triangle boxes reach the frame's outer
        two pixels). No `reverse`. Async on the current stream, no host wait."""
        fr, v, idx, flags = self._frames_args(frames, vertices, image_index)
        if mapping not in ("bilinear", "nearest"):
            raise ValueError(f"mapping: 'bilinear' or 'nearest', got {mapping!r}")
        if indexing not in ("corner", "reference"):
            raise ValueError(f"indexing: 'corner' or 'reference', got {indexing!r}")
        dtypes = {torch.float32: _lib.DTYPE_F32, torch.uint8: _lib.DTYPE_U8}
        tex = textures
        if not isinstance(tex, Tensor) or tex.dtype not in dtypes or tex.ndim not in (3, 4) or not tex.is_contiguous() or tex.device != self.torch_device:
            raise ValueError(f"textures: expected a contiguous float32 or uint8 tensor with 3 or 4 dims on {self.torch_device}, got "
                             f"{getattr(tex, 'dtype', type(tex))} {tuple(getattr(tex, 'shape', ()))} on {getattr(tex, 'device', None)}")
        if tex.ndim == 4 and tex.shape[0] != v.shape[0]:
            raise ValueError(f"textures: {tex.shape[0]} textures for {v.shape[0]} heads")
        th, tw, tc = tex.shape[-3:]
        _lib.check(self._lib.dad3d_mesh_render_texture_frames(
            self._handle, fr.device.data_ptr(), fr.host.ctypes.data, len(fr), v.data_ptr(), tex.data_ptr(), dtypes[tex.dtype],
            int(tex.ndim == 4), th, tw, tc, 0 if mapping == "nearest" else 1,
            _lib.TEX_INDEX_REFERENCE if indexing == "reference" else _lib.TEX_INDEX_CORNER, idx.data_ptr(), v.shape[0], flags.data_ptr(),
            self._stream()))
        return flags

    # -- lighting ----------------------------------------------------------------------------------
    def phong_light(self, vertices: Tensor, normals: Optional[Tensor] = None, ambient: float = 0.3, directional: float = 0.6,
                    specular: float = 0.1, specular_exp: float = 5, color_ambient: Sequence[float] = (1, 1, 1),
                    color_directional: Sequence[float] = (1, 1, 1), light_pos: Sequence[float] = (0, 0, 5),
                    view_pos: Sequence[float] = (0, 0, 5), normals_out: Optional[Tensor] = None) -> Tensor:
        """Per-vertex Phong light (lighting.py:41-62). `normals=None`: the vertex normals are computed in the same
        launch (and stored into `normals_out` when given) -- RenderPipeline's `_get_normal` + lighting in one pass."""
        v = self._verts(vertices)
        cfg = _lib.LightC(float(ambient), float(directional), float(specular), float(specular_exp),
                          (C.c_float * 3)(*color_ambient), (C.c_float * 3)(*color_directional),
                          (C.c_float * 3)(*light_pos), (C.c_float * 3)(*view_pos))
        out = torch.empty_like(v)
        if normals is None:
            n_out = None if normals_out is None else self._verts(normals_out, "normals_out")
            if n_out is not None and n_out.shape[0] != v.shape[0]:
                raise ValueError("normals_out: batch mismatch")
            _lib.check(self._lib.dad3d_mesh_normal_phong_light(self._handle, out.data_ptr(), None if n_out is None else n_out.data_ptr(),
                                                               v.data_ptr(), v.shape[0], C.byref(cfg), self._stream()))
            return out
        n = self._verts(normals, "normals")
        if n.shape[0] != v.shape[0]:
            raise ValueError("normals: batch mismatch")
        _lib.check(self._lib.dad3d_mesh_phong_light(self._handle, out.data_ptr(), v.data_ptr(), n.data_ptr(), v.shape[0],
                                                    C.byref(cfg), self._stream()))
        return out

    def render(self, vertices: Tensor, bg: Tensor, depth: Optional[Tensor] = None, reverse: bool = False,
               light_out: Optional[Tensor] = None, clear: bool = False, ambient: float = 0.3, directional: float = 0.6, specular: float = 0.1,
               specular_exp: float = 5, color_ambient: Sequence[float] = (1, 1, 1), color_directional: Sequence[float] = (1, 1, 1),
               light_pos: Sequence[float] = (0, 0, 5), view_pos: Sequence[float] = (0, 0, 5)) -> Tensor:
        """RenderPipeline.__call__ (lighting.py:37-71, texture=None) for a batch in TWO launches: the raster's geometry
        kernel also computes normals + Phong light (into `light_out`, allocated when None), the tile kernel rasterises
        with it into the 3-channel `bg`. Same results as `phong_light(v, None)` followed by `rasterize`. `clear=True`:
        `bg` is only a destination, rendered onto black (the geometry launch zeroes it: no fill launch in front)."""
        v = self._verts(vertices)
        img = _chk(bg, torch.uint8, 4, "bg", self.torch_device)
        if img.shape[-1] != 3:
            raise ValueError("render needs a 3-channel image (the light has three components)")
        if img.shape[0] != v.shape[0]:
            raise ValueError("bg: batch mismatch")
        light = torch.empty_like(v) if light_out is None else self._verts(light_out, "light_out")
        if light.shape[0] != v.shape[0]:
            raise ValueError("light_out: batch mismatch")
        if depth is not None and tuple(depth.shape) != tuple(img.shape[:3]):
            raise ValueError("depth: expected [B, h, w] like bg")
        cfg = _lib.LightC(float(ambient), float(directional), float(specular), float(specular_exp),
                          (C.c_float * 3)(*color_ambient), (C.c_float * 3)(*color_directional),
                          (C.c_float * 3)(*light_pos), (C.c_float * 3)(*view_pos))
        dptr = None if depth is None else _chk(depth, torch.float32, 3, "depth", self.torch_device).data_ptr()
        _lib.check(self._lib.dad3d_mesh_render(self._handle, img.data_ptr(), v.data_ptr(), light.data_ptr(), dptr, v.shape[0],
                                               img.shape[1], img.shape[2], C.byref(cfg), int(bool(reverse)) | (2 if clear else 0),
                                               self._stream()))
        return img
