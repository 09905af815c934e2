"""Shared by the render-texture tests and the golden generator: the reference's own `_render_texture_core`
(Sim3DR/lib/rasterize_kernel.cpp:358-463) called through ctypes, and the inputs the cases are made of.

The oracle recipe compiles the whole of rasterize_kernel.cpp into oracle/_ref/libsim3dr_ref.so, which exports the function
under its C++ name (the reference's Cython binding comments it out, so there is no other way in). TEST INFRASTRUCTURE."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libsim3dr_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_texture_golden.npz")
# void _render_texture_core(float* image, float* vertices, int* triangles, float* texture, float* tex_coords, int* tex_triangles,
#                           float* depth_buffer, int nver, int tex_nver, int ntri, int h, int w, int c, int tex_h, int tex_w,
#                           int tex_c, int mapping_type)
SYMBOL = "_Z20_render_texture_corePfS_PiS_S_S0_S_iiiiiiiiii"
_F, _I = C.POINTER(C.c_float), C.POINTER(C.c_int)


def ref_available() -> bool:
    return os.path.isfile(REF_LIB)


_fn = None


def _core():
    global _fn
    if _fn is None:
        fn = getattr(C.CDLL(REF_LIB), SYMBOL)
        fn.restype = None
        fn.argtypes = [_F, _F, _I, _F, _F, _I, _F] + [C.c_int] * 10
        _fn = fn
    return _fn


def ref_render(vertices, triangles, texture, tex_coords, tex_triangles, h, w, c, mapping_type, image=None, depth=None):
    """The compiled reference on one image. tex_coords [T,3] float32 (its stride), texture [tex_h,tex_w,tex_c] float32.
    Returns (image float32 [h,w,c], depth float32 [h,w]); `image` / `depth` are the starting contents (zeros / -1e8)."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    v, t, tex, tc, tt = f32(vertices), i32(triangles), f32(texture), f32(tex_coords), i32(tex_triangles)
    assert v.ndim == 2 and v.shape[1] == 3 and t.shape == tt.shape and t.shape[1] == 3 and tc.ndim == 2 and tc.shape[1] == 3 and tex.ndim == 3
    assert t.size == 0 or (t.min() >= 0 and t.max() < len(v) and t.max() < len(tc) and tt.min() >= 0 and tt.max() < len(tc))
    assert 1 <= c <= tex.shape[2]
    img = np.zeros((h, w, c), np.float32) if image is None else f32(image).copy()
    dep = np.full((h, w), -1e8, np.float32) if depth is None else f32(depth).copy()
    assert img.shape == (h, w, c) and dep.shape == (h, w)
    p = lambda a, ty: a.ctypes.data_as(ty)  # noqa: E731
    _core()(p(img, _F), p(v, _F), p(t, _I), p(tex, _F), p(tc, _F), p(tt, _I), p(dep, _F), len(v), len(tc), len(t), h, w, c,
            tex.shape[0], tex.shape[1], tex.shape[2], int(mapping_type))
    return img, dep


def unrolled(vertices, triangles, tex_coords2, tex_triangles):
    """Corner indexing stated in the reference's terms: one vertex and one texture coordinate per triangle corner. The
    reference called on this mesh reads x AND y of a corner from that corner's row, which is what corner indexing means."""
    t = np.asarray(triangles).reshape(-1)
    v = np.ascontiguousarray(np.asarray(vertices, np.float32)[t])
    tri = np.arange(len(t), dtype=np.int32).reshape(-1, 3)
    tc = np.zeros((len(t), 3), np.float32)
    tc[:, :2] = np.asarray(tex_coords2, np.float32)[np.asarray(tex_triangles).reshape(-1), :2]
    return v, tri, tc, tri.copy()


def band_mask(h, w):
    """The two-pixel border band of rasterize_kernel.cpp:423."""
    y, x = np.mgrid[0:h, 0:w]
    return (x < 2) | (x > w - 3) | (y < 2) | (y > h - 3)


def head_vertices(static, h, w, shift_x=0.0, fill=0.8):
    """The packaged FLAME template scaled into an h x w frame (y down, the larger z towards the viewer, as Sim3DR wants it)."""
    t = np.asarray(static["template_geo"], np.float64)
    lo, hi = t.min(0), t.max(0)
    s = fill * min(h, w) / max(hi[0] - lo[0], hi[1] - lo[1])
    c = 0.5 * (lo + hi)
    v = np.empty_like(t)
    v[:, 0] = (t[:, 0] - c[0]) * s + 0.5 * w + shift_x
    v[:, 1] = -(t[:, 1] - c[1]) * s + 0.5 * h
    v[:, 2] = (t[:, 2] - c[2]) * s
    return v.astype(np.float32)


def head_texcoords(static, size):
    """Per-vertex texel coordinates [V,3] = (x, y, 0) of the synthetic cylindrical layout for a size x size texture."""
    from dad_3dheads_amd import synthetic
    from dad_3dheads_amd.uv_texture import texel_coords

    tc = np.zeros((len(static["template_geo"]), 3), np.float32)
    tc[:, :2] = texel_coords(synthetic.synthetic_texcoords(size, static)["vt"], size)
    return tc


def smooth_texture(h, w, c, seed):
    """A float texture with distinct values per texel and channel, in [0, 255]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255.0 / max(w - 1, 1)), (y * 255.0 / max(h - 1, 1)), ((x + y) % 16) * 16.0, (x * y) % 251 * 1.0][:c] +
                    [np.zeros((h, w))] * max(c - 4, 0), -1)
    return np.clip(base * 0.9 + rng.uniform(0, 25, (h, w, c)), 0, 255).astype(np.float32)
