"""The expected results of the occlusion-aware texture bake on the CPU. TEST INFRASTRUCTURE.

`expected_depth_frames`          `UVMap.depth_frames`: per head the window of its box in the frame it names, computed in float32, and
                                 the oracle's `rasterize_triangles` (the reference's own `_rasterize_triangles` where oracle/_ref holds
                                 it, else the C port pinned to it) on the head with z negated, on the frame's h x w canvas, negated
                                 back, `+inf` where no triangle covers, cropped to the window.
`expected_bake_frames_occluded`  `UVMap.bake_frames(occlusion="self")` / `TextureAccumulator(occlusion="self").add`: the candidate arrays
                                 of `uv_texture_restatement` (point, normal, n_dot_view in float64), the two tests of the reference, the
                                 third test in float64 against the expected depth maps, then the plain bake or "best view wins" exactly
                                 as `texture_frames_restatement.expected_bake_frames` states them.
`two_planes`                     the hand-made mesh of two parallel squares with its hand-written atlas."""
import hashlib

import numpy as np

import uv_texture_restatement as R

BAKE_FLAG_INDEX, BAKE_FLAG_DEPTH_WINDOW, BAKE_FLAG_NONFINITE = 1, 2, 4


def expected_window(hw, v, depth_side):
    """(flag, [x0, y0, ww, wh]) of one head `v [V,3]` float32 against a frame of `hw = (h, w)`, in float32 like the kernel."""
    v = np.asarray(v, np.float32)
    if not np.isfinite(v).all():
        return BAKE_FLAG_NONFINITE, [0, 0, 0, 0]
    h, w = hw
    lo, hi = v.min(0), v.max(0)
    fx0, fx1 = max(np.floor(lo[0]), np.float32(0)), min(np.ceil(hi[0]), np.float32(w - 1))
    fy0, fy1 = max(np.floor(lo[1]), np.float32(0)), min(np.ceil(hi[1]), np.float32(h - 1))
    if fx0 > fx1 or fy0 > fy1:
        return 0, [0, 0, 0, 0]  # outside its frame: an ordinary outcome
    ww, wh = int(fx1 - fx0 + 1), int(fy1 - fy0 + 1)
    if ww > depth_side or wh > depth_side:
        return BAKE_FLAG_DEPTH_WINDOW, [0, 0, 0, 0]
    return 0, [int(fx0), int(fy0), ww, wh]


def expected_depth_frames(oracle, frames_hw, vertices, faces, image_index, depth_side):
    """frames_hw: (h, w) per frame; vertices [N,V,3] float32. -> (maps, window int32 [N,4], flags int32 [N]): maps[k] is the float32
    array [wh, ww] of head k's window (None for a flagged head), entry [j, i] the depth at pixel (x0 + i, y0 + j)."""
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    index = np.asarray(image_index).reshape(-1)
    n = len(vertices)
    maps, window, flags = [], np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    for k in range(n):
        f = int(index[k])
        v = np.ascontiguousarray(vertices[k], dtype=np.float32)
        if not 0 <= f < len(frames_hw):
            flags[k] = BAKE_FLAG_INDEX | (0 if np.isfinite(v).all() else BAKE_FLAG_NONFINITE)
            maps.append(None)
            continue
        h, w = frames_hw[f]
        flags[k], window[k] = expected_window((h, w), v, depth_side)
        if flags[k]:
            maps.append(None)
            continue
        x0, y0, ww, wh = window[k].tolist()
        if ww == 0:
            maps.append(np.zeros((0, 0), np.float32))
            continue
        negated = v.copy()
        negated[:, 2] = -negated[:, 2]
        depth, tri_buf, _ = oracle.rasterize_triangles(negated, faces, h, w)
        full = np.where(tri_buf >= 0, -depth, np.float32(np.inf)).astype(np.float32)
        maps.append(full[y0:y0 + wh, x0:x0 + ww].copy())
    return maps, window, flags


_CANDIDATES = {}


def candidates(texture_data, v, faces):
    """Per candidate, in float64 as the reference computes them: point [n,3], normal [n,3] and texel [n]. Kept per (atlas, head)."""
    v = np.asarray(v, np.float64)
    key = (id(texture_data), hashlib.sha1(v.tobytes()).hexdigest())
    if key not in _CANDIDATES:
        td = texture_data
        vf, bc, ids, s = td["valid_pixel_3d_faces"], td["valid_pixel_b_coords"], td["valid_pixel_ids"], td["img_size"]
        p = v[vf[:, 0], :] * bc[:, 0][:, None] + v[vf[:, 1], :] * bc[:, 1][:, None] + v[vf[:, 2], :] * bc[:, 2][:, None]
        n = R.vertex_normals(v, faces)
        pn = n[vf[:, 0], :] * bc[:, 0][:, None] + n[vf[:, 1], :] * bc[:, 1][:, None] + n[vf[:, 2], :] * bc[:, 2][:, None]
        texel = (td["y_coords"][ids].astype(int) % s) * s + (td["x_coords"][ids].astype(int) % s)
        _CANDIDATES[key] = (p, pn, texel)
    return _CANDIDATES[key]


def _last_writer(ok, texel, n_tex):
    win = np.full(n_tex, -1, np.int64)
    idx = np.flatnonzero(ok)
    t = texel[idx]
    last = len(t) - 1 - np.unique(t[::-1], return_index=True)[1]
    win[t[last]] = idx[last]
    return win


def three_tests(texture_data, hw, v, faces, depth_map, window, depth_bias, slope_bias):
    """-> (accepted, hidden, p, ndv, texel): the candidates that pass the reference's two tests, and those of them the depth test hides."""
    p, pn, texel = candidates(texture_data, v, faces)
    h, w = hw
    ndv = -pn[:, 2]
    x0, y0, ww, wh = [int(t) for t in window]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rxy = np.round(p[:, :2])
        accepted = ~(ndv < 0.0) & (rxy[:, 0] > 0) & (rxy[:, 0] < w) & (rxy[:, 1] > 0) & (rxy[:, 1] < h)
        d = np.full(len(p), np.inf)
        ix, iy = np.where(accepted, rxy[:, 0], 0).astype(np.int64) - x0, np.where(accepted, rxy[:, 1], 0).astype(np.int64) - y0
        inside = accepted & (ix >= 0) & (ix < ww) & (iy >= 0) & (iy < wh)
        d[inside] = depth_map[iy[inside], ix[inside]].astype(np.float64)
        hidden = accepted & (p[:, 2] > d + (depth_bias + slope_bias * ((np.abs(pn[:, 0]) + np.abs(pn[:, 1])) / ndv)))
    return accepted, hidden, p, ndv, texel


def expected_bake_frames_occluded(texture_data, frames, vertices, faces, image_index, depth_maps, window, depth_flags, depth_bias=1.0,
                                  slope_bias=1.0, textures=None, score=None):
    """`texture_frames_restatement.expected_bake_frames` with the third test. depth_maps / window / depth_flags: what
    `expected_depth_frames` returned for the same heads. -> (textures, score or None, flags, stats); stats[k] = None for a flagged head,
    else the texel counts of `expected_bake_frames` (on the winners after the depth test) plus `accepted` (candidates that pass the two
    tests), `hidden` (of those, the ones failing only the depth test) and `moved` (texels whose winner changed to another candidate)."""
    s = int(texture_data["img_size"])
    n = len(vertices)
    index = np.asarray(image_index).reshape(-1)
    accumulate = score is not None
    tex = np.array(textures, np.uint8).reshape(n, s * s, 3).copy() if accumulate else np.zeros((n, s * s, 3), np.uint8)
    sc = np.array(score, np.float32).reshape(n, s * s).copy() if accumulate else None
    flags = np.zeros(n, np.int32)
    stats = []
    for k in range(n):
        f = int(index[k])
        flags[k] = int(depth_flags[k]) | (0 if 0 <= f < len(frames) else BAKE_FLAG_INDEX)
        if flags[k]:
            stats.append(None)
            continue
        frame = frames[f]
        h, w = frame.shape[:2]
        accepted, hidden, p, ndv, texel = three_tests(texture_data, (h, w), vertices[k], faces, depth_maps[k], window[k], depth_bias, slope_bias)
        before, win = _last_writer(accepted, texel, s * s), _last_writer(accepted & ~hidden, texel, s * s)
        has = np.flatnonzero(win >= 0)
        cand = win[has]
        xy = np.round(p[cand, :2]).astype(int)
        pix = frame[xy[:, 1], xy[:, 0]]
        st = dict(candidates=len(has), accepted=int(accepted.sum()), hidden=int(hidden.sum()),
                  moved=int(((win >= 0) & (before >= 0) & (win != before)).sum()), lost=int(((win < 0) & (before >= 0)).sum()),
                  replaced=0, kept=0, first=0)
        if not accumulate:
            tex[k, has] = pix
        else:
            s_new = ndv[cand].astype(np.float32)
            old = sc[k, has]
            with np.errstate(invalid="ignore"):
                rep = s_new > old  # strict: a tie keeps the older sample; a NaN never replaces
            held = old > -1.0
            st.update(replaced=int((rep & held).sum()), kept=int((~rep & held).sum()), first=int((rep & ~held).sum()))
            tex[k, has[rep]] = pix[rep]
            sc[k, has[rep]] = s_new[rep]
        stats.append(st)
    return tex.reshape(n, s, s, 3), (sc.reshape(n, s, s) if accumulate else None), flags, stats


def two_planes():
    """Two parallel squares facing the viewer (normals (0, 0, -1)): the front one at z = 0 over x in 10..20, the back one at z = 5 over x
    in 10..30, both over y in 10..20; 8 vertices, 4 triangles. The hand-written atlas (8 x 8 texels, one candidate each) puts
    texels 0..3 on the front square, 8..11 on the back square UNDER the front one and 16..19 on the back square BESIDE it.
    -> (vertices float32 [8,3], faces int32 [4,3], texture_data, groups) with groups = dict(front=, under=, beside=) of texel ids."""
    v = np.array([[10, 10, 0], [10, 20, 0], [20, 10, 0], [20, 20, 0], [10, 10, 5], [10, 20, 5], [30, 10, 5], [30, 20, 5]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 5, 7]], np.int32)
    # (triangle, barycentrics) -> the point: front (13, 13) (12, 15) | (18, 16) (17, 18); under (14, 12) (12, 14) | (16, 18) (18, 17);
    # beside (24, 11) (22, 13) | (26, 18) (28, 16)
    rows = [(0, (0.4, 0.3, 0.3)), (0, (0.3, 0.5, 0.2)), (1, (0.4, 0.2, 0.4)), (1, (0.2, 0.3, 0.5)),
            (2, (0.6, 0.2, 0.2)), (2, (0.5, 0.4, 0.1)), (3, (0.2, 0.7, 0.1)), (3, (0.3, 0.6, 0.1)),
            (2, (0.2, 0.1, 0.7)), (2, (0.1, 0.3, 0.6)), (3, (0.2, 0.2, 0.6)), (3, (0.4, 0.1, 0.5))]
    texels = [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19]
    size = 8
    td = dict(img_size=size, valid_pixel_ids=np.asarray(texels, np.int64),
              x_coords=(np.arange(size * size) % size).astype(np.float64), y_coords=(np.arange(size * size) // size).astype(np.float64),
              valid_pixel_3d_faces=np.asarray([faces[t] for t, _ in rows], np.int64),
              valid_pixel_b_coords=np.asarray([b for _, b in rows], np.float64))
    return v, faces, td, dict(front=texels[0:4], under=texels[4:8], beside=texels[8:12])
