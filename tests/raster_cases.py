"""The adversarial meshes of the raster tests, and what the frames chain must do with them, in plain NumPy. TEST INFRASTRUCTURE.

`PROFILES`, `build_case`   the eight profiles of test_gpu_raster_fuzz.py / test_gpu_raster_alpha.py (moved here unchanged: the same seed and
                           profile give the same arrays, pinned by tests/golden/raster_cases_digest.json).
`tri_boxes`, `tile_entries`  the screen box of rasterize_kernel.cpp:246-254 and the number of (64 x 64 tile, triangle) entries a head needs.
`admitted`                 the flags of the frames chain's admission rule as include/dad3d.h documents it.
`scene`                    three heads of one topology in three frames of different sizes.
`whole_box_frames`         one frame-covering triangle per frame, for every box width 1..64 inside a tile.
`directed_pairs`           hand-made pairs of overlapping flat triangles: mixed signs, the two zeros, thresholds, a zero-area triangle.
`tiny_atlas`               a hand-made atlas for `UVMap` on any faces (only the faces matter to the depth maps).

Nothing here reads a kernel: the box and the admission rule are written from the reference and the header, so a test that predicts flags
with them predicts them on the CPU. tests/test_raster_cases_host.py certifies on the reference alone that every case reaches what it claims."""
import hashlib

import numpy as np

PROFILES = ("pixel_centres", "slivers", "tie_planes", "tile_straddle", "mixed_sizes", "split_tile", "wild", "layers")
SEEDS = (1, 2, 3, 4)  # the scenes of the GPU tests: four per profile
DIGEST_SEEDS = (1, 20247)
TILE = 64
FRAME_FLAG_INDEX, FRAME_FLAG_CAPACITY = 1, 2  # DAD3D_FRAME_FLAG_* of include/dad3d.h


def build_case(seed: int, profile: str):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(40, 200)), int(rng.integers(40, 280))
    if profile == "split_tile":
        h, w = 128, 192
    nver = int(rng.integers(6, 120))
    ntri = int(rng.integers(4, 260))
    v = np.empty((nver, 3), np.float32)
    v[:, 0] = rng.uniform(-12, w + 12, nver)
    v[:, 1] = rng.uniform(-12, h + 12, nver)
    v[:, 2] = rng.uniform(-4, 4, nver)
    t = rng.integers(0, nver, (ntri, 3)).astype(np.int32)
    if profile == "pixel_centres":  # every vertex on a pixel centre, half-integer depths: edges run through pixel centres
        v[:, :2] = np.round(v[:, :2])
        v[:, 2] = np.round(v[:, 2] * 2) / 2
    elif profile == "slivers":  # collinear and nearly collinear corners, repeated corners, tiny areas
        base = rng.integers(0, nver, ntri)
        d = rng.uniform(-30, 30, (ntri, 2)).astype(np.float32)
        extra = nver + 2 * ntri
        v2 = np.empty((extra, 3), np.float32)
        v2[:nver] = v
        for k in range(ntri):
            a = v[base[k]]
            e = float(rng.choice([0.0, 1e-6, 1e-4, 1e-2, 0.3]))
            v2[nver + 2 * k] = [a[0] + d[k, 0], a[1] + d[k, 1], a[2] + 1]
            v2[nver + 2 * k + 1] = [a[0] + 2 * d[k, 0] - e * d[k, 1], a[1] + 2 * d[k, 1] + e * d[k, 0], a[2] - 1]
        t = np.stack([base, nver + 2 * np.arange(ntri), nver + 2 * np.arange(ntri) + 1], 1).astype(np.int32)
        t[::7, 2] = t[::7, 1]  # a repeated corner: exactly zero area
        v, nver = v2, extra
    elif profile == "tie_planes":  # constant-depth planes: every overlap is an exact tie, decided by the triangle index
        v[:, 2] = np.round(v[:, 2])
        v[rng.integers(0, nver, nver // 2), 2] = 1.0
    elif profile == "tile_straddle":  # corners hugging the 64-pixel tile borders and the image edge
        snap = rng.choice([0.0, 63.0, 64.0, 127.0, 128.0, float(w - 1), float(w)], nver)
        v[:, 0] = snap + rng.choice([-1.0, -0.5, -1e-3, 0.0, 1e-3, 0.5, 1.0], nver) + rng.uniform(-3, 3, nver) * (rng.random(nver) < 0.5)
        snap = rng.choice([0.0, 63.0, 64.0, float(h - 1), float(h)], nver)
        v[:, 1] = snap + rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], nver) + rng.uniform(-40, 40, nver) * (rng.random(nver) < 0.5)
        v = v.astype(np.float32)
    elif profile == "mixed_sizes":  # a few image-sized triangles among many small ones, equal depths between the two kinds
        near = rng.integers(0, nver, ntri)
        t = np.stack([near, (near + 1) % nver, (near + 2) % nver], 1).astype(np.int32)
        order = np.argsort(v[:, 0] // 6 * 1000 + v[:, 1])
        v = v[order]
        big = np.array([[-50, -50, 0.5], [w + 60, -40, 0.5], [w / 2, h + 90, 0.5], [-30, h + 20, -0.5]], np.float32)
        v = np.concatenate([v, big]).astype(np.float32)
        t = np.concatenate([t, np.array([[nver, nver + 1, nver + 2], [nver + 3, nver + 1, nver + 2], [nver, nver + 2, nver + 3]], np.int32)])
        v[: nver // 3, 2] = 0.5
        nver += 4
    elif profile == "split_tile":  # one tile far beyond the split threshold: 2x2 and 4x4 parts, lists re-classed per part
        nver, ntri = 400, 900
        v = np.empty((nver, 3), np.float32)
        v[:, 0] = rng.uniform(60, 132, nver)
        v[:, 1] = rng.uniform(-4, 70, nver)
        v[:, 2] = np.round(rng.uniform(-3, 3, nver))
        t = rng.integers(0, nver, (ntri, 3)).astype(np.int32)
    elif profile == "layers":  # sheets of opposite winding over the same pixels, tile lists long enough for the two-pass
        # path of the tile kernel (far-facing triangles culled against what the near-facing ones left): exact depth ties
        # between the sheets, sheets that cross, either winding in front, a sheet of mixed winding, a pre-filled depth buffer
        h, w = int(rng.integers(70, 140)), int(rng.integers(70, 200))
        g = int(rng.integers(12, 18))
        sheets_v, sheets_t = [], []
        level = rng.permutation([0.0, 0.0, 1.0, -1.0])[:3]  # two sheets may share a depth plane
        for k in range(3):
            gx, gy = np.meshgrid(np.linspace(-4, w * rng.uniform(0.6, 1.05), g), np.linspace(-4, h * rng.uniform(0.6, 1.05), g))
            jit = rng.uniform(-1.2, 1.2, (2,) + gx.shape) * (rng.random(gx.shape) < 0.7)
            px, py = gx + jit[0], gy + jit[1]
            if k == 1:
                px, py = np.round(px), np.round(py)
            z = level[k] + np.round(rng.uniform(-1, 1, gx.shape) * 2) / 2 * (rng.random(gx.shape) < 0.4) + float(rng.choice([0.0, 0.02])) * gx
            sv = np.stack([px.ravel(), py.ravel(), z.ravel()], 1)
            i = (np.arange(g - 1)[:, None] * g + np.arange(g - 1)[None]).ravel()
            st_ = np.concatenate([np.stack([i, i + 1, i + g], 1), np.stack([i + 1, i + g + 1, i + g], 1)])
            if k == 1:
                st_ = st_[:, ::-1]
            if k == 2:
                flip = rng.random(len(st_)) < 0.5
                st_[flip] = st_[flip][:, ::-1]
            sheets_t.append(st_ + sum(len(q) for q in sheets_v))
            sheets_v.append(sv)
        v = np.concatenate(sheets_v).astype(np.float32)
        t = np.concatenate(sheets_t).astype(np.int32)
        t = t[rng.permutation(len(t))]
        nver = len(v)
    elif profile == "wild":  # huge and non-finite-producing coordinates next to ordinary ones
        v[rng.integers(0, nver, 3), 0] = rng.choice([1e7, -1e7, 3e38, -3e38, 65535.5])
        v[rng.integers(0, nver, 2), 1] = rng.choice([1e7, -3e38])
        v[rng.integers(0, nver, 2), 2] = rng.choice([3e38, -3e38, 1e-40])
    c = int(rng.choice([1, 3, 3, 4]))
    col = rng.uniform(-0.2, 1.2, (nver, c)).astype(np.float32)  # colours a little outside [0, 1]: the (uchar) cast wraps
    bg = rng.integers(0, 255, (h, w, c)).astype(np.uint8)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t), col, bg, h, w, bool(rng.integers(0, 2))


def case_digest(case) -> str:
    """sha256 over everything `build_case` returned: dtype, shape and bytes of each array, the repr of each scalar."""
    m = hashlib.sha256()
    for item in case:
        if isinstance(item, np.ndarray):
            m.update(f"{item.dtype.str}{item.shape}".encode())
            m.update(np.ascontiguousarray(item).tobytes())
        else:
            m.update(repr((type(item).__name__, item)).encode())
    return m.hexdigest()


# ---- the box of the reference and the tiles it touches --------------------------------------------------------------------------------
def f2i_x86(a):
    """`(int)` of a float as the reference's x86-64 build converts it (cvttss2si): truncation, INT_MIN for NaN and out of range."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        inside = (a >= np.float32(-2147483648.0)) & (a < np.float32(2147483648.0))
        return np.where(inside, np.trunc(np.where(inside, a, 0)).astype(np.int64), -(2**31))


def _std_min(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(b < a, b, a)  # std::min(a, b)


def _std_max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a)  # std::max(a, b)


def tri_boxes(v, t, h, w):
    """rasterize_kernel.cpp:246-254 for every triangle -> (x_min, x_max, y_min, y_max, visible): int64 arrays [ntri], the pixel box
    clipped to the h x w frame, and whether the reference walks it (`x_max < x_min || y_max < y_min` -> continue)."""
    p = np.asarray(v, np.float32)[np.asarray(t)]
    x, y = p[:, :, 0], p[:, :, 1]
    x_min = np.maximum(f2i_x86(np.ceil(_std_min(x[:, 0], _std_min(x[:, 1], x[:, 2])))), 0)
    x_max = np.minimum(f2i_x86(np.floor(_std_max(x[:, 0], _std_max(x[:, 1], x[:, 2])))), w - 1)
    y_min = np.maximum(f2i_x86(np.ceil(_std_min(y[:, 0], _std_min(y[:, 1], y[:, 2])))), 0)
    y_max = np.minimum(f2i_x86(np.floor(_std_max(y[:, 0], _std_max(y[:, 1], y[:, 2])))), h - 1)
    return x_min, x_max, y_min, y_max, ~((x_max < x_min) | (y_max < y_min))


def _longest_run_in_a_tile(lo, hi):
    """The most pixels of [lo, hi] that one tile column (or row) holds."""
    t0, t1 = lo // TILE, hi // TILE
    return np.where(t0 == t1, hi - lo + 1, np.where(t1 - t0 >= 2, TILE, np.maximum(TILE - lo % TILE, hi % TILE + 1)))


def tile_entries(v, t, h, w):
    """-> (entries, over32, over64): the (tile, triangle) entries the head needs when each visible triangle's clipped box is listed in
    every 64 x 64 tile it touches, and how many visible triangles have more than 32 / more than 64 pixels of their box in some tile."""
    x0, x1, y0, y1, vis = tri_boxes(v, t, h, w)
    x0, x1, y0, y1 = x0[vis], x1[vis], y0[vis], y1[vis]
    tiles = (x1 // TILE - x0 // TILE + 1) * (y1 // TILE - y0 // TILE + 1)
    most = _longest_run_in_a_tile(x0, x1) * _longest_run_in_a_tile(y0, y1)
    return int(tiles.sum()), int((most > 32).sum()), int((most > 64).sum())


def pool_entries(ntri, n_heads):
    """The list pool of a call, include/dad3d.h: 4 * ntri * N entries."""
    return 4 * int(ntri) * int(n_heads)


def admitted(needs, image_index, n_frames, pool):
    """The flags of the frames chain (include/dad3d.h, DAD3D_FRAME_FLAG_*): INDEX for a head whose index names no frame (it needs no
    entries); nobody else is dropped if all heads fit the pool together; otherwise the heads take their entries in ascending order and a
    head that no longer fits gets CAPACITY and takes none."""
    index = np.asarray(image_index).reshape(-1).tolist()
    has_frame = [0 <= f < n_frames for f in index]
    need = [int(n) if ok else 0 for n, ok in zip(needs, has_frame)]
    flags = [0 if ok else FRAME_FLAG_INDEX for ok in has_frame]
    if sum(need) <= pool:
        return flags
    used = 0
    for k, ok in enumerate(has_frame):
        if not ok:
            continue
        if need[k] > pool - used:
            flags[k] = FRAME_FLAG_CAPACITY
        else:
            used += need[k]
    return flags


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
_INDEXES = ([0, 0, 1], [0, 2, 0], [2, 1, 2], [1, 0, 0], [2, 2, 0], [0, 0, 2])


def scene(seed: int, profile: str) -> dict:
    """Three heads of one topology (`build_case(seed, profile)`: its points, the same points under reversed indices, and a third set on
    shifted pixel centres, as test_batch_of_three_different_adversarial_meshes builds them) with three-channel colours, in three frames:
    frame 0 -- the case's own canvas, a side that is a multiple of 64 made one pixel longer; frame 1 -- exactly 64 x 64; frame 2 -- another
    size of at most 280 a side, to be given to the device as a strided view at an odd address (`view`: its index). Two heads share a frame.
    -> dict(t, verts [3,nver,3], cols [3,nver,3], bgs, image_index, view, reverse)."""
    v, t, _, _, h, w, rev = build_case(seed, profile)
    rng = np.random.default_rng([seed, PROFILES.index(profile), 77])
    v2 = v[::-1].copy()
    v3 = v.copy()
    v3[:, :2] = np.round(v3[:, :2] + rng.uniform(-3, 3, v3[:, :2].shape))
    v3[:, 2] = np.round(v3[:, 2])
    verts = np.stack([v, v2, v3]).astype(np.float32)
    cols = rng.uniform(-0.2, 1.2, verts.shape).astype(np.float32)
    h0, w0 = h + (h % TILE == 0), w + (w % TILE == 0)
    h2, w2 = int(rng.integers(33, 281)), int(rng.integers(33, 281))
    while (h2, w2) == (h0, w0) or (h2, w2) == (TILE, TILE):
        h2 += 1
    shapes = [(h0, w0), (TILE, TILE), (h2, w2)]
    bgs = [rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8) for fh, fw in shapes]
    index = list(_INDEXES[int(rng.integers(0, len(_INDEXES)))])
    return dict(t=t, verts=verts, cols=cols, bgs=bgs, image_index=index, view=2, reverse=rev, profile=profile, seed=seed)


def scene_needs(sc):
    """-> (needs [3], over32 [3], over64 [3]) of the scene's heads, each against the frame it names."""
    out = []
    for k, f in enumerate(sc["image_index"]):
        h, w = sc["bgs"][f].shape[:2]
        out.append(tile_entries(sc["verts"][k], sc["t"], h, w))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def scene_flags(sc):
    needs, _, _ = scene_needs(sc)
    return admitted(needs, sc["image_index"], len(sc["bgs"]), pool_entries(len(sc["t"]), len(sc["verts"])))


# ---- every box width inside a tile ----------------------------------------------------------------------------------------------------
WHOLE_BOX_BG = 255


def whole_box_frames() -> dict:
    """Frames of bh x bw pixels for every bw in 1..64 with bh in {1, 63, 64}, and frames of 64 x (64 + bw): their second tile starts at
    pixel 64 and is bw wide. One topology of a single triangle; head k is one triangle that strictly contains its whole frame, with
    vertices off the pixel grid, a depth that varies over it and a colour per corner inside (0.05, 0.9), so that no drawn byte is the
    background's 255 and a pixel computed at the wrong place takes a visibly different colour. The clipped box of the triangle is the
    whole tile part: every p < bw * bh of the walk is visited. In every seventh frame a second head of the same shape lies BEHIND the first
    and comes later. -> dict(t, verts [N,3,3], cols [N,3,3], shapes, image_index)."""
    rng = np.random.default_rng(64)
    shapes = [(bh, bw) for bh in (1, 63, 64) for bw in range(1, TILE + 1)] + [(TILE, TILE + bw) for bw in range(1, TILE + 1)]
    verts, cols, index = [], [], []

    def cover(h, w, z):
        a, b = rng.uniform(2.1, 9.9, 2)
        tri = np.array([[-a, -b, z[0]], [3 * w + 10.3 + a, -b + 0.25, z[1]], [-a + 0.25, 3 * h + 10.7 + b, z[2]]], np.float32)
        return tri[rng.permutation(3)]  # either winding, any first corner

    for f, (h, w) in enumerate(shapes):
        verts.append(cover(h, w, rng.uniform(-3, 3, 3)))
        cols.append(rng.uniform(0.05, 0.9, (3, 3)).astype(np.float32))
        index.append(f)
    for f in range(0, len(shapes), 7):
        h, w = shapes[f]
        verts.append(cover(h, w, rng.uniform(-30, -20, 3)))
        cols.append(rng.uniform(0.05, 0.9, (3, 3)).astype(np.float32))
        index.append(f)
    return dict(t=np.array([[0, 1, 2]], np.int32), verts=np.stack(verts).astype(np.float32), cols=np.stack(cols), shapes=shapes,
                image_index=index)


# ---- directed pairs -------------------------------------------------------------------------------------------------------------------
BELOW_1E8 = float(np.nextafter(np.float32(1e8), np.float32(0)))
ABOVE_M1E8 = float(np.nextafter(np.float32(-1e8), np.float32(0)))
DEPTH_PAIRS = {"mixed_signs": (-1.0, 1.0), "two_zeros": (-0.0, 0.0), "both_negative": (-3.0, -2.0), "threshold": (1e8, BELOW_1E8)}
FRAME_PAIRS = {"mixed_signs": (-1.0, 1.0), "two_zeros": (-0.0, 0.0), "both_negative": (-3.0, -2.0), "threshold": (-1e8, ABOVE_M1E8)}
PAIR_SIDES = (4, 12)  # clipped boxes of 16 and of 144 pixels: a lane's walk and the whole wave's in both kernels
PAIR_FRAME = (24, 40)


def directed_pair(za, zb, side, swap=False, zero_area=False):
    """Two flat right triangles of 6 vertices in a 24 x 40 frame, each with a clipped box of side x side pixels, B one pixel to the right of
    A so that they share pixels: triangle A at depth za, triangle B at zb; `swap` lists B first. `zero_area`: B has a repeated corner and
    its box is a run of pixels that starts inside A (the depth raster's `u >= 0 && v >= 0 && u + v < 1` takes u = v = 0 as inside: it
    covers its box; the frames raster's strict test never does).
    -> (vertices [6,3] float32, triangles [2,3] int32, colours [6,3] float32, flat per triangle)."""
    leg = side - 0.25
    a = np.array([[5.5, 3.5, za], [5.5 + leg, 3.75, za], [5.75, 3.5 + leg, za]], np.float32)  # box x 6 .. 5 + side, y 4 .. 3 + side
    b = a + np.array([1.0, 0.0, 0.0], np.float32)
    b[:, 2] = zb
    if zero_area:
        b = np.array([[7.0, 5.0, zb], [5.0 + side, 5.0, zb], [5.0 + side, 5.0, zb]], np.float32)
    v = np.concatenate([b, a] if swap else [a, b])
    col = np.repeat(np.array([[0.2, 0.4, 0.6], [0.9, 0.7, 0.1]], np.float32)[[1, 0] if swap else [0, 1]], 3, 0)
    return v, np.arange(6, dtype=np.int32).reshape(2, 3), np.ascontiguousarray(col)


def directed_pairs(table):
    """Every pair of `table` (DEPTH_PAIRS or FRAME_PAIRS) and the zero-area case, in both triangle orders, at both box sizes.
    -> list of (name, vertices, colours); the triangles are always [[0,1,2],[3,4,5]]."""
    out = []
    for side in PAIR_SIDES:
        for swap in (False, True):
            for name, (za, zb) in table.items():
                v, _, col = directed_pair(za, zb, side, swap)
                out.append((f"{name} side {side} swap {swap}", v, col))
            v, _, col = directed_pair(1.5, -2.5, side, swap, zero_area=True)
            out.append((f"zero_area zb = -2.5 side {side} swap {swap}", v, col))
            v, _, col = directed_pair(1.5, 2.5, side, swap, zero_area=True)
            out.append((f"zero_area zb = 2.5 side {side} swap {swap}", v, col))
    return out


PAIR_TRIANGLES = np.arange(6, dtype=np.int32).reshape(2, 3)


def tiny_atlas(faces, size=8):
    """A hand-written atlas like `texture_occlusion_restatement.two_planes`'s for any faces: one candidate at the centroid of each of the
    first size * size faces. The depth maps read the faces only."""
    f = np.asarray(faces).reshape(-1, 3)[: size * size]
    n = len(f)
    return dict(img_size=size, valid_pixel_ids=np.arange(n, dtype=np.int64),
                x_coords=(np.arange(size * size) % size).astype(np.float64), y_coords=(np.arange(size * size) // size).astype(np.float64),
                valid_pixel_3d_faces=f.astype(np.int64), valid_pixel_b_coords=np.full((n, 3), 1.0 / 3.0))
