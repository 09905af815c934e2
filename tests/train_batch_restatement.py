"""Float64 / float32 NumPy restatement of the training-batch chain of csrc/train_batch.hip and dataset.FlameBatchBuilder, and
the seeded scenes the golden, the tests and the benchmark share. Never reads the reference tree.

  project        _load_mesh + _project_vertices_onto_image (flame_dataset.py:115-141), fp32, sequential k sums
  landmarks68    get_68_landmarks on the world vertices ((c0 w0 + c1 w1) + c2 w2, fp32), then w := 1 (:151-157)
  presence       0 < x < w and 0 < y < h in crop pixels (:167-170)
  albu_keypoints albumentations 1.0.0 LongestMaxSize + PadIfNeeded / Resize on "xy" keypoints, float64 as under the pinned
                 numpy 1.22 (np.float32 * Python float is float64 there), rounded to fp32 once (:189-190)
  chain          the whole of gt_keypoints_kernel in its fixed order; a subset id outside [0, nver) gives a NaN row, absent
  chain64        the same chain in float64 with no fp32 rounding: the plain high-precision reference
"""
from __future__ import annotations

import numpy as np

from dad_3dheads_amd.resize_geometry import longest_max_size

N_VERTS = 5023


# ---- the chain -----------------------------------------------------------------------------------------------------------
def _mat_points(m: np.ndarray, p: np.ndarray) -> np.ndarray:
    """m [4,4] . p[:, k] for k = 0..3 summed in order, fp32 (the kernel's order; numpy's sgemm may fuse or reorder)."""
    m = m.astype(np.float32)
    out = np.empty_like(p, dtype=np.float32)
    for i in range(4):
        out[:, i] = ((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3] * p[:, 3]
    return out


def world(vertices: np.ndarray, model_view: np.ndarray) -> np.ndarray:
    v = np.asarray(vertices, np.float32)
    return _mat_points(model_view, np.concatenate([v, np.ones_like(v[:, :1])], 1))


def rows(world_h: np.ndarray, ids) -> np.ndarray:
    """world_h[ids], with a NaN row for every id outside [0, nver): the kernel reads nothing there (include/dad3d.h)."""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(world_h))
    out = np.full(ids.shape + (4,), np.nan, world_h.dtype)
    out[ok] = world_h[ids[ok]]
    return out


def landmarks68(world_h: np.ndarray, corners: np.ndarray, weights: np.ndarray) -> np.ndarray:
    tri = rows(world_h, corners)[..., :3]  # [68,3 corners,3]
    w = weights.astype(np.float32)
    xyz = (tri[:, 0] * w[:, 0, None] + tri[:, 1] * w[:, 1, None]) + tri[:, 2] * w[:, 2, None]
    return np.concatenate([xyz, np.ones_like(xyz[:, :1])], 1).astype(np.float32)


def project(world_h: np.ndarray, projection: np.ndarray, height: int, crop_x: int, crop_y: int) -> np.ndarray:
    c = _mat_points(projection, world_h)
    x, y = c[:, 0] / c[:, 3], c[:, 1] / c[:, 3]
    return np.stack([x - np.float32(crop_x), (np.float32(height) - y) - np.float32(crop_y)], -1).astype(np.float32)


def presence(xy: np.ndarray, w: int, h: int) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (0 < xy[:, 0]) & (xy[:, 0] < w) & (0 < xy[:, 1]) & (xy[:, 1] < h)


def albu_keypoints(xy: np.ndarray, h: int, w: int, size: int, mode: str) -> np.ndarray:
    """fp32 crop-pixel points -> fp32 points of the size x size network input."""
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    if mode == "longest_max_size":
        s = size / max([h, w])  # LongestMaxSize.apply_to_keypoint: a Python float
        _, _, top, left = longest_max_size(h, w, size)  # PadIfNeeded's pads on the resized image
        return np.stack([x * s + left, y * s + top], -1).astype(np.float32)
    return np.stack([x * (size / w), y * (size / h)], -1).astype(np.float32)


def chain(vertices, model_view, projection, frame, size, mode, index=None, corners=None, weights=None):
    """One item: frame = (image height, crop x, y, w, h) -> (full [N,2], subset_px [K,2], subset_norm [K,2], presence [K]).
    A subset id outside [0, N) gives a NaN row that is absent; with neither index nor corners the subset is empty."""
    height, cx, cy, w, h = (int(v) for v in frame[:5])
    wh = world(vertices, model_view)
    if index is None and corners is None:
        sub = wh[:0]
    else:
        sub = landmarks68(wh, corners, weights) if index is None else rows(wh, index)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        xy_sub, xy_full = project(sub, projection, height, cx, cy), project(wh, projection, height, cx, cy)
        pres = presence(xy_sub, w, h)
        sub_px = albu_keypoints(xy_sub, h, w, size, mode)
        return albu_keypoints(xy_full, h, w, size, mode), sub_px, (sub_px / np.float32(size)).astype(np.float32), pres


def chain64(vertices, model_view, projection, frame, size, mode, index=None, corners=None, weights=None):
    """`chain` in float64 throughout, nothing rounded to fp32 on the way: the plain high-precision reference. Float64 outputs."""
    height, cx, cy, w, h = (int(v) for v in frame[:5])
    v = np.asarray(vertices, np.float64)
    wh = np.concatenate([v, np.ones_like(v[:, :1])], 1) @ np.asarray(model_view, np.float64).T
    if index is None and corners is None:
        sub = wh[:0]
    elif index is None:
        xyz = (rows(wh, corners)[..., :3] * np.asarray(weights, np.float64)[:, :, None]).sum(1)
        sub = np.concatenate([xyz, np.ones_like(xyz[:, :1])], 1)
    else:
        sub = rows(wh, index)
    out = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for pts in (wh, sub):
            c = pts @ np.asarray(projection, np.float64).T
            xy = np.stack([c[:, 0] / c[:, 3] - cx, (height - c[:, 1] / c[:, 3]) - cy], -1)
            if mode == "longest_max_size":
                _, _, top, left = longest_max_size(h, w, size)
                out.append((xy, xy * (size / max(h, w)) + (left, top)))
            else:
                out.append((xy, xy * (size / w, size / h)))
        (_, full), (xy_sub, sub_px) = out
        return full, sub_px, sub_px / size, presence(xy_sub, w, h)


# ---- seeded scenes ------------------------------------------------------------------------------------------------------
def image(seed: int, h: int, w: int) -> np.ndarray:
    """A seeded uint8 RGB image: smooth gradients plus noise (the resize taps see structure, not only noise)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], -1)
    return ((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def rotation(rng, max_deg: float) -> np.ndarray:
    a = np.deg2rad(rng.uniform(-max_deg, max_deg, 3))
    cx, cy, cz, sx, sy, sz = *np.cos(a), *np.sin(a)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def mesh(seed: int, template: np.ndarray) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (template + rng.normal(0, 2e-3, template.shape)).astype(np.float32)


def camera(seed: int, img_h: int, img_w: int, head_px: float, centre_px):
    """(model_view, projection) float32: a posed head at z ~ -1 in front of a pixel-space pinhole camera whose head spans
    about head_px pixels around centre_px (x right, y up in the image, as the reference flips it with H - y)."""
    rng = np.random.default_rng(seed)
    z = -rng.uniform(0.8, 1.2)
    f = head_px * -z / 0.2  # the FLAME head is ~0.2 units across
    mv = np.eye(4)
    mv[:3, :3] = rotation(rng, 25)
    mv[:3, 3] = (rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), z)
    cx, cy = centre_px[0], img_h - centre_px[1]
    pm = np.array([[f, 0, -cx, 0], [0, f, -cy, 0], [0, 0, -1.0, -0.1], [0, 0, -1.0, 0]])
    return mv.astype(np.float32), pm.astype(np.float32)


def crop_sides(rng, n: int) -> np.ndarray:
    """The benchmark's crop sides: log-uniform in [64, 640] px (DAD-3DHeads face boxes span small to large faces)."""
    return np.exp(rng.uniform(np.log(64), np.log(640), (n, 2))).astype(np.int64)


def ortho_edge_vertices(verts: np.ndarray, bbox, img_h: int, subset_ids) -> np.ndarray:
    """An orthographic item (identity model-view and projection: image x = X, image y = H - Y exactly): the mesh scaled into
    the crop, and the vertices of the first six subset ids moved onto the crop's edges and one pixel inside them. In index
    mode those keypoints lie exactly on the edges (absent) or exactly inside (present)."""
    x, y, w, h = (int(v) for v in bbox)
    v = (verts * np.float32(100) + np.float32([x + w / 2, img_h - (y + h / 2), 0])).astype(np.float32)
    edge = [(x, img_h - (y + 5)), (x + w, img_h - (y + 7)), (x + 9, img_h - y), (x + 11, img_h - (y + h)), (x + 1, img_h - (y + 1)),
            (x + w - 1, img_h - (y + h - 1))]
    for j, (ex, ey) in enumerate(edge):
        v[subset_ids[j]] = (ex, ey, 0.5)
    return v


# ---- the golden's cases, rebuilt from their seeds -------------------------------------------------------------------------
def lmk68_tables(static):
    from dad_3dheads_amd.benchmark_export import embedding_path

    with np.load(embedding_path()) as z:
        return static["faces"].astype(np.int64)[z["face_idx"]], z["b_coords"].astype(np.float32)


def subset_ids(subset: str, static) -> np.ndarray:
    return static["lmk_445"] if subset == "445" else lmk68_tables(static)[0][:, 0]


def case_config(z, name: str, kp_dir: str = "", static=None) -> dict:
    """The dataset config of a golden case; index mode writes its list under kp_dir (load_2d_indices' layout)."""
    import os

    subset = str(z[name + "_subset"])
    if subset == "445":
        os.makedirs(kp_dir, exist_ok=True)
        np.save(os.path.join(kp_dir, "keypoints_445.npy"), {"all": [int(v) for v in static["lmk_445"]]})
        kp = {"2d_subset_name": "keypoints_445", "2d_subset_path": kp_dir}
    else:
        kp = {"2d_subset_name": "multipie_keypoints", "2d_subset_path": kp_dir}
    return {"img_size": 256, "stride": 4, "num_classes": 68 if subset == "68" else 445, "keypoints": kp,
            "transform": {"normalize": str(z[name + "_normalize"]), "resize_mode": str(z[name + "_mode"])}}


def case_items(z, name: str, static) -> list:
    """Raw items (dataset.FlameDataset.__getitem__'s form) of a golden case: the crops of its recorded bboxes."""
    p = name + "_"
    ids = subset_ids(str(z[p + "subset"]), static)
    items = []
    for i, seed in enumerate(z[p + "seeds"]):
        shape = tuple(int(v) for v in z[p + "image_shapes"][i])
        x, y, w, h = (int(v) for v in z[p + "bbox"][i])
        verts = mesh(int(seed), static["template_geo"])
        if str(z[p + "kinds"][i]) == "ortho_edges":
            verts = ortho_edge_vertices(verts, (x, y, w, h), shape[0], ids)
        assert np.float64(verts).sum() == z[p + "vertices_sum"][i], (name, i)
        img = image(int(seed), *shape[:2])
        items.append({"image": np.ascontiguousarray(img[y: y + h, x: x + w]), "bbox": np.array([x, y, w, h], np.int32),
                      "image_shape": np.array(shape, np.int64), "vertices": verts, "model_view": z[p + "model_view"][i],
                      "projection": z[p + "projection"][i], "SAMPLE_INDEX_KEY": i, "IMAGE_FILENAME_KEY": f"img_{seed}.png"})
    return items
