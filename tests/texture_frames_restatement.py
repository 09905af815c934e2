"""The expected results of the texture-of-tracked-heads entries on the CPU. TEST INFRASTRUCTURE.

`expected_bake_frames`      `UVMap.bake_frames` / `TextureAccumulator.add`: per head `uv_texture_restatement.winning_candidates` on the
                            frame the head names (the frame's own h and w), then either the plain bake or the "best view wins" rule
                            with `ndv.astype(np.float32)` and a strict `>`.
`expected_textured_frames`  `Mesh.render_texture_frames`: per frame, per head in ascending head index, one call of the reference's own
                            `_render_texture_core` (render_texture_ref.ref_render) on `image = frame.astype(float32)` with a fresh depth
                            buffer, then `.astype(uint8)`. Needs the compiled reference (oracle/_ref)."""
import numpy as np

import render_texture_ref as RT
from uv_texture_restatement import winning_candidates

BAKE_FLAG_INDEX = 1


def expected_bake_frames(texture_data, frames, vertices, faces, image_index, textures=None, score=None):
    """frames: uint8 arrays [H,W,3]; vertices [N,V,3] float32; image_index [N]. `score=None`: the plain bake. Otherwise `textures`
    [N,S,S,3] and `score` [N,S,S] are the state before the call (left as they are). -> (textures, score or None, flags, stats):
    stats[k] = None for a flagged head, else a dict of texel counts: `candidates` (texels with a winner), `replaced` (held a sample
    and took the new one), `kept` (held a sample and kept it), `first` (filled for the first time), `inside` / `outside` (front-facing
    candidates that pass / fail the frame's strict bounds)."""
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
        if not 0 <= f < len(frames):
            flags[k] = BAKE_FLAG_INDEX
            stats.append(None)
            continue
        frame = frames[f]
        h, w = frame.shape[:2]
        win, p, ndv, _ = winning_candidates(texture_data, frame, np.asarray(vertices[k], np.float64), faces)
        has = np.flatnonzero(win >= 0)
        cand = win[has]
        xy = np.round(p[cand, :2]).astype(int)
        pix = frame[xy[:, 1], xy[:, 0]]
        with np.errstate(invalid="ignore"):
            front = ~(ndv < 0.0)
            rxy = np.round(p[:, :2])
            inside = (rxy[:, 0] > 0) & (rxy[:, 0] < w) & (rxy[:, 1] > 0) & (rxy[:, 1] < h)
        st = dict(candidates=len(has), inside=int((front & inside).sum()), outside=int((front & ~inside).sum()), replaced=0, kept=0, first=0)
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


def expected_textured_frames(frames, vertices, triangles, textures, tex_coords, tex_triangles, image_index, mapping_type, indexing="corner",
                             skip=()):
    """frames: uint8 arrays [H,W,3] (left as they are) -> new arrays, drawn. textures [N,th,tw,tc] or one shared [th,tw,tc], any
    dtype with values a float32 holds. tex_coords [T,2 or 3] in texel units. `indexing="corner"` is stated in the reference's terms
    through `render_texture_ref.unrolled`; "reference" calls it as it is (tex_coords [T,3]). Heads in `skip` (what a test found
    flagged) and heads that name no frame are skipped."""
    out = [np.ascontiguousarray(f).copy() for f in frames]
    tex = np.asarray(textures)
    for k, f in enumerate(np.asarray(image_index).reshape(-1).tolist()):
        if k in skip or not 0 <= f < len(out):
            continue
        t = (tex[k] if tex.ndim == 4 else tex).astype(np.float32)
        h, w = out[f].shape[:2]
        if indexing == "corner":
            v, tri, tc, tt = RT.unrolled(vertices[k], triangles, tex_coords, tex_triangles)
        else:
            v, tri, tc, tt = vertices[k], triangles, tex_coords, tex_triangles
        img, _ = RT.ref_render(v, tri, t, tc, tt, h, w, 3, mapping_type, image=out[f].astype(np.float32))
        out[f] = img.astype(np.uint8)
    return out
