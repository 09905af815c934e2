"""The expected frames of `Mesh.rasterize_frames` / `Mesh.render_frames` on the CPU: per frame, per head in ascending head index,
one call of the reference's `rasterize(vertices[k], triangles, colors[k], bg=frame)` (Sim3DR/Sim3DR.py:14-29) through
`oracle.sim3dr_ref.Sim3DROracle` -- every call with a z-buffer of its own, so a later head paints over an earlier one. A head whose
index names no frame is skipped, and so are the heads in `skip` (what a test found flagged)."""
import numpy as np

from oracle.sim3dr_ref import phong_light_ref


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def expected_frames(oracle, frames, vertices, triangles, colors, image_index, reverse=False, skip=()):
    """frames: uint8 arrays [H,W,3] (left as they are) -> new arrays, drawn."""
    out = [np.ascontiguousarray(f).copy() for f in frames]
    for k, f in enumerate(np.asarray(image_index).reshape(-1).tolist()):
        if k in skip or not 0 <= f < len(out):
            continue
        oracle.rasterize(_c(vertices[k]), triangles, _c(colors[k]), bg=out[f], reverse=reverse)
    return out


def head_light(oracle, vertices, triangles, **light):
    """RenderPipeline's per-vertex light of every head (lighting.py:64-67): `_get_normal`, then the numpy Phong terms."""
    with np.errstate(all="ignore"):
        return np.stack([phong_light_ref(oracle.get_normal(_c(v), triangles), _c(v), **light) for v in vertices]).astype(np.float32)


def expected_lit_frames(oracle, frames, vertices, triangles, image_index, reverse=False, **light):
    lights = head_light(oracle, vertices, triangles, **light)
    return expected_frames(oracle, frames, vertices, triangles, lights, image_index, reverse=reverse), lights


def coverage(oracle, shape, vertices, triangles, image_index, frame):
    """bool [H,W]: the pixels of `frame` some head of it draws (a fragment passed `>` against -1e8)."""
    h, w = shape
    cover = np.zeros((h, w), bool)
    for k, f in enumerate(np.asarray(image_index).reshape(-1).tolist()):
        if f != frame:
            continue
        _, depth = oracle.rasterize(_c(vertices[k]), triangles, np.zeros_like(_c(vertices[k])), height=h, width=w, channel=3, return_depth=True)
        cover |= depth > -1e8
    return cover
