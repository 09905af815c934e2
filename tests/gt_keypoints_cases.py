"""Shared by tests/test_train_batch_host.py and tests/test_gpu_gt_keypoints.py: the inputs of `dad3d_gt_keypoints` that both run, so
that the CPU certifies (against mutated restatements of the chain) the inputs the GPU test feeds to the kernel. Pure NumPy.

A case is a dict: name, vertices [B,nver,3], model_view [B,4,4], projection [B,4,4] float32, frames [B,8] int32 (image height, crop
x, y, w, h, pad_top, pad_left, 0), size, mode, and the subset: index [K] int32, or corners [K,3] int32 + weights [K,3] float32, or
neither (K = 0). Optional: presence [B,K] bool written by hand; clean (the same subset with every bad id replaced by a good one) and
bad [K] bool (the rows a bad id poisons)."""
import functools
import itertools

import numpy as np

import train_batch_restatement as rs
from dad_3dheads_amd import synthetic
from dad_3dheads_amd.resize_geometry import longest_max_size

F = np.float32
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
SUBSETS, MODES, SIZES = ("index", "barycentric"), ("longest_max_size", "resize"), (256, 255, 300)
# (nver, K): one point; the last vertex in the last lane of block 0 (68 + 188 = 256) and in the first lane of block 1; no subset; no
# vertex, so that every id is out of range; subset lanes and vertex lanes sharing block 1; the builder's two shapes
SHAPES = ((1, 1), (188, 68), (189, 68), (256, 0), (0, 5), (300, 445), (5023, 68), (5023, 445))


@functools.lru_cache(maxsize=None)
def static():
    return synthetic.load_static()


def frame_rows(boxes, size):
    """[(image height, x, y, w, h)] -> frames [B,8] with the pads of LongestMaxSize + PadIfNeeded at `size`."""
    out = np.zeros((len(boxes), 8), np.int32)
    for i, (height, x, y, w, h) in enumerate(boxes):
        _, _, top, left = longest_max_size(h, w, size)
        out[i] = (height, x, y, w, h, top, left, 0)
    return out


def subset(kind, nver, k, rng):
    """The subset arguments of a case. The packaged tables name vertices up to 3868 and serve nver = 5023 only; elsewhere the ids
    are drawn in [0, nver) (nver = 0: in [0, 5), all out of range) and the weights are the packaged embedding's rows, cycled."""
    if k == 0:
        return {}
    corners68, weights68 = rs.lmk68_tables(static())
    if kind == "index":
        if nver == rs.N_VERTS and k in (68, 445):
            return {"index": rs.subset_ids(str(k), static()).astype(np.int32)}
        return {"index": rng.integers(0, nver or 5, k).astype(np.int32)}
    weights = np.ascontiguousarray(weights68[np.arange(k) % len(weights68)])
    if nver == rs.N_VERTS and k == 68:
        return {"corners": corners68.astype(np.int32), "weights": weights}
    return {"corners": rng.integers(0, nver or 5, (k, 3)).astype(np.int32), "weights": weights}


# image (h, w), head size in px, head centre, crop (x, y, w, h): a negative corner with w > h; a 1-px-wide crop; h > w
SCENES = (((480, 640), 150.0, (35.0, 40.0), (-13, -7, 200, 150)),
          ((720, 1280), 260.0, (600.0, 350.0), (598, 230, 1, 220)),
          ((333, 257), 200.0, (140.0, 150.0), (85, 80, 97, 180)))


def posed(kind, mode, size, nver, k, seed=0, scenes=SCENES):
    rng = np.random.default_rng([seed, nver, k, size])
    cams = [rs.camera(seed + 10 * i + 1, *shape, head, centre) for i, (shape, head, centre, _) in enumerate(scenes)]
    verts = np.stack([rs.mesh(seed + 10 * i + 2, static()["template_geo"])[:nver] for i in range(len(scenes))])
    case = {"name": f"posed-{kind}-{mode}-{size}-{nver}-{k}", "vertices": verts.reshape(len(scenes), nver, 3),
            "model_view": np.stack([c[0] for c in cams]), "projection": np.stack([c[1] for c in cams]),
            "frames": frame_rows([(shape[0], *crop) for shape, _, _, crop in scenes], size), "size": size, "mode": mode}
    case.update(subset(kind, nver, k, rng))
    return case


@functools.lru_cache(maxsize=None)
def posed_cases():
    return tuple(posed(kind, mode, size, nver, k) for kind, mode, size, (nver, k) in itertools.product(SUBSETS, MODES, SIZES, SHAPES))


@functools.lru_cache(maxsize=None)
def batch_case():
    """B = 70 items of 40 vertices and 7 keypoints: the item axis of the grid. Every item has its own camera and its own crop, laid
    over the middle of its projected vertices so that present and absent keypoints mix."""
    rng = np.random.default_rng(70)
    scenes = []
    for _ in range(70):
        h, w = (int(v) for v in rng.integers(200, 900, 2))
        scenes.append(((h, w), float(rng.uniform(100, 600)), (w / 2, h / 2), (0, 0, 1, 1)))
    case = posed("barycentric", "resize", 255, 40, 7, seed=1000, scenes=tuple(scenes))
    boxes = []
    for b, ((h, _), _, _, _) in enumerate(scenes):
        xy = rs.project(rs.world(case["vertices"][b], case["model_view"][b]), case["projection"][b], h, 0, 0)
        cw, ch = (int(v) for v in rng.integers(1, 200, 2))
        mid = np.median(xy, 0) - rng.uniform(0.2, 0.8, 2) * (cw, ch)
        boxes.append((h, int(np.floor(mid[0])), int(np.floor(mid[1])), cw, ch))
    return dict(case, name="batch-70", frames=frame_rows(boxes, 255))


def homogeneous_case(kind):
    """World rows with w = 2 (the whole model-view doubled, which is exact) under a projection whose last column is not zero: index
    mode carries the homogeneous row as it is, 68-landmark mode sets w := 1 after the combination, and the two differ."""
    case = posed(kind, "longest_max_size", 256, 300, 68, seed=50)
    case["model_view"] = case["model_view"] * F(2)
    case["projection"] = case["projection"].copy()
    case["projection"][:, 0, 3], case["projection"][:, 1, 3] = 30.0, -20.0
    return dict(case, name=f"homogeneous-{kind}")


# ---- exact crop edges ------------------------------------------------------------------------------------------------------
def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


EDGE_W, EDGE_H = 97, 180  # a non-square crop: longest_max_size pads its short side, the width


def edge_points():
    """(x, y, present) in crop pixels; the presence column is written by hand: 0 < x < w and 0 < y < h, strictly."""
    w, h = EDGE_W, EDGE_H
    return [
        (0.0, 10.5, False), (-0.0, 10.5, False), (up(0), 10.5, True), (down(0), 10.5, False),        # the left edge
        (w, 10.5, False), (down(w), 10.5, True), (up(w), 10.5, False),                               # the right edge
        (20.25, 0.0, False), (20.25, -0.0, False), (20.25, up(0), True), (20.25, down(0), False),    # the top edge
        (20.25, h, False), (20.25, down(h), True), (20.25, up(h), False),                            # the bottom edge
        (1.0, 1.0, True), (w - 1, h - 1, True), (0.0, 0.0, False), (w, h, False), (up(0), up(0), True), (down(w), down(h), True),
        (up(0), h, False), (w, down(h), False),
        # one pixel outside the short side: resized, x = left + s * (-1) and left + s * (w + 1) lie inside (0, size)
        (-1.0, 90.0, False), (w + 1, 90.0, False),
        (48.0, -1.0, False), (48.0, h + 1, False), (48.0, 90.0, True),
    ]


def _exact_corners(t, pattern):
    """Three fp32 values whose combination with WEIGHTS[pattern] is `t` exactly (checked where the case is built)."""
    t = F(t)
    whole = t == np.floor(t) and abs(t) >= 16
    if pattern == 0:
        return (t, F(3.0), F(-5.0))
    if pattern == 1:
        return (t - F(8), t + F(8), F(7.0)) if whole else (F(2) * t, F(0.0), F(7.0))
    return (t - F(4), t + F(4), t) if whole else (F(0.0), F(0.0), F(2) * t)


WEIGHTS = np.array([(1, 0, 0), (0.5, 0.5, 0), (0.25, 0.25, 0.5)], F)


def edge_case(kind, mode, size):
    """Identity matrices, image height 0, crop corner 0: the crop-pixel point of a vertex (X, Y, Z) is (X, -Y) exactly."""
    pts = edge_points()
    xy = np.array([(x, y) for x, y, _ in pts], F)
    k = len(pts)
    if kind == "index":
        order = np.random.default_rng(3).permutation(k)
        verts = np.zeros((k, 3), F)
        verts[order] = np.stack([xy[:, 0], -xy[:, 1], np.linspace(-1, 1, k, dtype=F)], -1)
        sub = {"index": order.astype(np.int32)}
    else:
        verts = np.zeros((k, 3, 3), F)
        for j in range(k):  # x and y of a row share the row's weight triple
            verts[j, :, 0] = _exact_corners(xy[j, 0], j % 3)
            verts[j, :, 1] = _exact_corners(-xy[j, 1], j % 3)
            verts[j, :, 2] = (0.5, -0.25, 0.125)
        weights = WEIGHTS[np.arange(k) % 3]
        verts = verts.reshape(k * 3, 3)
        sub = {"corners": np.arange(k * 3, dtype=np.int32).reshape(k, 3), "weights": weights}
        got = rs.landmarks68(rs.world(verts, np.eye(4, dtype=F)), sub["corners"], weights)
        assert np.array_equal(got[:, 0], xy[:, 0]) and np.array_equal(got[:, 1], -xy[:, 1]), "the combination is not exact"
    eye = np.eye(4, dtype=F)[None]
    return dict({"name": f"edges-{kind}-{mode}-{size}", "vertices": verts[None], "model_view": eye, "projection": eye,
                 "frames": frame_rows([(0, 0, 0, EDGE_W, EDGE_H)], size), "size": size, "mode": mode,
                 "presence": np.array([[p for _, _, p in pts]], bool), "points": xy}, **sub)


@functools.lru_cache(maxsize=None)
def edge_cases():
    return tuple(edge_case(kind, mode, size) for kind, mode, size in itertools.product(SUBSETS, MODES, (256, 255)))


# ---- ids out of range ------------------------------------------------------------------------------------------------------
def bad_id_case(kind):
    """Each bad id between good neighbours. `clean` is the same subset with a good id in each bad place."""
    case = posed(kind, "longest_max_size", 256, 40, 9, seed=20)
    ids = (-1, 40, INT32_MAX, INT32_MIN)
    bad = np.zeros(9, bool)
    if kind == "index":
        clean = case["index"].copy()
        dirty = clean.copy()
        dirty[1::2] = ids
        bad[1::2] = True
        case.update(index=dirty, clean={"index": clean})
    else:
        clean = case["corners"].copy()
        dirty = clean.copy()
        for row, pos, v in ((1, 0, -1), (3, 1, 40), (5, 2, INT32_MAX), (7, 0, INT32_MIN)):  # one bad corner of three, in each place
            dirty[row, pos] = v
            bad[row] = True
        case.update(corners=dirty, clean={"corners": clean, "weights": case["weights"]})
    return dict(case, name=f"bad-ids-{kind}", bad=bad)


@functools.lru_cache(maxsize=None)
def bad_id_cases():
    return tuple(bad_id_case(kind) for kind in SUBSETS)


# ---- the camera plane ------------------------------------------------------------------------------------------------------
def camera_plane_case(kind):
    """The points of test_gpu_projection.test_points_behind_and_on_the_camera_plane as subset points: identity rotation and z
    translation -1, so clip w = -(z - 1) exactly. Item 0 is that camera; item 1 has an infinity in its model-view, item 2 one in
    its projection. 68-landmark mode names each vertex three times with dyadic weights, so the combination is the vertex."""
    mv, pm = rs.camera(7, 480, 640, 200.0, (320, 240))
    mv[:3, :3] = np.eye(3, dtype=F)
    mv[:3, 3] = (0, 0, -1)
    tiny = F(1) - F(2.0 ** -23)
    v = np.array([[0.05, 0.02, 0.0],      # in front: w = 1
                  [0.05, 0.02, 1.5],      # behind: w = -0.5, a mirrored point
                  [0.05, -0.02, 1.0],     # on the plane: (+inf, -inf before the flip)
                  [-0.05, 0.0, 1.0],      # on the plane: (-inf, NaN)
                  [0.0, 0.0, 1.0],        # on the plane, on the axis: (NaN, NaN)
                  [1.0, -1.0, tiny],      # w = 2^-23
                  [-1.0, 1.0, tiny]], F)
    mvs, pms = np.stack([mv, mv, mv]), np.stack([pm, pm, pm])
    mvs[1, 0, 3] = np.inf
    pms[2, 0, 0] = -np.inf
    n = len(v)
    if kind == "index":
        sub = {"index": np.arange(n, dtype=np.int32)[::-1].copy()}
    else:
        sub = {"corners": np.repeat(np.arange(n, dtype=np.int32)[::-1], 3).reshape(n, 3), "weights": np.tile(F([0.5, 0.25, 0.25]), (n, 1))}
    return dict({"name": f"camera-plane-{kind}", "vertices": np.stack([v, v, v]), "model_view": mvs, "projection": pms,
                 "frames": frame_rows([(480, -3, 4, 640, 480)] * 3, 256), "size": 256, "mode": "longest_max_size"}, **sub)


@functools.lru_cache(maxsize=None)
def special_cases():
    return tuple(f(kind) for f in (camera_plane_case, homogeneous_case) for kind in SUBSETS)


def all_cases():
    return posed_cases() + (batch_case(),) + edge_cases() + bad_id_cases() + special_cases()


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- what the kernel must give ---------------------------------------------------------------------------------------------
def subset_of(case):
    return {k: case[k] for k in ("index", "corners", "weights") if k in case}


def n_subset(case):
    return len(case.get("index", case.get("corners", ())))


def evaluate(case, chain=rs.chain, sub=None):
    """`chain` on every item -> (full [B,nver,2], subset_px [B,K,2], subset_norm [B,K,2], presence [B,K])."""
    sub = subset_of(case) if sub is None else sub
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # the camera-plane cases divide by zero on purpose
        out = [chain(case["vertices"][b], case["model_view"][b], case["projection"][b], case["frames"][b], case["size"], case["mode"], **sub)
               for b in range(len(case["frames"]))]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


_expected = {}


def expected(case):
    """`rs.chain` of a case, computed once and shared by the tests; the arrays are read-only."""
    if case["name"] not in _expected:
        out = evaluate(case)
        for a in out:
            a.setflags(write=False)
        _expected[case["name"]] = out
    return _expected[case["name"]]


def same_bits(got, want):
    """Equal as uint32 words, NaNs in the same places (a NaN's payload is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
