"""Shared by tests/test_pose_host.py and tests/test_gpu_head_pose.py: the seeded inputs, scipy as the reference of the numpy
statement in dad_3dheads_amd/pose.py, and the rule for which heads' arrow points may be compared coordinate by coordinate."""
import functools

import numpy as np
import torch

from dad_3dheads_amd import pose

EDGE_PX = 1e-6        # a coordinate this close to an integer before truncation, or to a half before rounding, may land on either side
EDGE_CAP = 0.01       # at most this share of the heads may be left out for it
RPY_TOL_DEG = 1e-9    # float64 spacing at 180 is 2.8e-14; a polar factor with singular values near 1 is well conditioned; 1 degree
#                       from the lock the first and third angle amplify errors at most ~57 times: four decades inside this bound
SEED = 20240607


@functools.lru_cache(maxsize=None)
def rot6_rows(n: int, seed: int = SEED) -> np.ndarray:
    """Seeded 6-D rotations as a network gives them: unnormalised, float32. Read-only (shared by the tests)."""
    rows = np.random.default_rng(seed).standard_normal((n, 6)).astype(np.float32)
    rows.setflags(write=False)
    return rows


def scipy_euler(matrices: np.ndarray) -> np.ndarray:
    from scipy.spatial.transform import Rotation

    return Rotation.from_matrix(np.asarray(matrices, dtype=np.float64)).as_euler("xyz", degrees=True)


def reference_rpy(rot6: np.ndarray) -> np.ndarray:
    """`overlay.calculate_rpy`'s rule on the float32 matrix of the numpy statement: scipy, then limit_angle."""
    angles = scipy_euler(np.transpose(pose.rotation_rows(rot6), (0, 2, 1)))
    return np.array([[pose.limit_angle(a[2]), pose.limit_angle(a[0] - 180.0), pose.limit_angle(a[1])] for a in angles])


def raw_points(rpy: np.ndarray, sizes) -> np.ndarray:
    """The statement's arrow points before truncation and rounding, float64 [n,10,2]; `sizes`: one (h, w) or one per head."""
    sizes = [sizes] * len(rpy) if isinstance(sizes[0], (int, np.integer)) else sizes
    return np.stack([pose.arrow_points(r, int(s[0]), int(s[1])) for r, s in zip(rpy, sizes)])


def edge_gap(raw: np.ndarray) -> np.ndarray:
    """float64 [n]: how far the head's closest coordinate lies from where its value jumps, in pixels: an end from an integer (it is
    truncated), a tip from a half (it is rounded)."""
    ends, tips = raw[:, 1:4], raw[:, 4:]
    end_gap = np.abs(ends - np.rint(ends)).min((1, 2))
    tip_gap = np.abs(np.abs(tips - np.floor(tips)) - 0.5).min((1, 2))
    return np.minimum(end_gap, tip_gap)


def near_edge(raw: np.ndarray) -> np.ndarray:
    """bool [n]: some end lies within EDGE_PX of an integer, or some tip within EDGE_PX of a half."""
    return edge_gap(raw) <= EDGE_PX


def assert_points(got: np.ndarray, rpy: np.ndarray, sizes, what: str) -> None:
    """`got` float32 [n,10,2] equals the statement's table for every head that is not near an edge; at most EDGE_CAP are."""
    raw = raw_points(rpy, sizes)
    skip = near_edge(raw)
    assert skip.mean() <= EDGE_CAP, (what, skip.mean())
    want = pose.snap_points(raw)
    bad = np.flatnonzero((got != want).any((1, 2)) & ~skip)
    assert bad.size == 0, (what, bad[:5], got[bad[:1]], want[bad[:1]])


def conditioned_rows(n: int, seed: int = SEED + 1) -> np.ndarray:
    """Rows with |v1| >= 0.1 and the angle between v1 and v2 at least 0.1 rad from 0 and pi."""
    rows = np.random.default_rng(seed).standard_normal((2 * n, 6)).astype(np.float32)
    v1, v2 = rows[:, :3].astype(np.float64), rows[:, 3:].astype(np.float64)
    cos = (v1 * v2).sum(1) / (np.linalg.norm(v1, axis=1) * np.linalg.norm(v2, axis=1))
    angle = np.arccos(np.clip(cos, -1.0, 1.0))
    keep = (np.linalg.norm(v1, axis=1) >= 0.1) & (angle >= 0.1) & (angle <= np.pi - 0.1)
    assert keep.sum() >= n
    return rows[keep][:n]


def lock_rows() -> np.ndarray:
    """6-D rotations whose transposed matrix is an exact lock matrix: rows (0, c, s), -+(0, -s, c), (-+1, 0, 0) -- a signed
    permutation block with a 2 x 2 rotation block -- so the second Euler angle is exactly +-90 degrees."""
    rows = []
    for sign in (1.0, -1.0):
        for deg in (0.0, 17.0, 90.0, 123.0, 180.0, 200.0, 305.5):
            c, s = np.float32(np.cos(np.radians(deg))), np.float32(np.sin(np.radians(deg)))
            b1 = np.array([0.0, c, s], np.float32)
            b2 = -sign * np.array([0.0, -s, c], np.float32)
            rows.append(np.concatenate([b1, b2]))
    rows = np.stack(rows).astype(np.float32)
    m = np.transpose(pose.rotation_rows(rows), (0, 2, 1))
    assert np.all(m[:, :2, 0] == 0) and np.all(m[:, 2, 1:] == 0) and np.all(np.abs(m[:, 2, 0]) == 1), "not exact lock matrices"
    return rows


PROCRUSTES_COUNTS = (2, 3, 7, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def procrustes_inputs(n_points: int, items: int = 12, seed: int = SEED + 2):
    """Noisy rotated, scaled and shifted copies: X, Y float64 [items,n,3]. For n >= 4 only items whose normalised covariance has
    its two smallest singular values summing to >= 0.1 are kept: then the polar factor's error is bounded by about eps * 10 * a
    hundred operations ~ 2e-13. Two points are collinear and three are coplanar once centred, so their covariance is singular
    whatever the values, and those counts are checked by the rule for planar and collinear sets."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(seed + n_points)
    many = 4 * items
    x = rng.standard_normal((many, n_points, 3)) * rng.uniform(0.5, 3.0, (many, 1, 3)) + 5.0 * rng.standard_normal((many, 1, 3))
    rot = Rotation.random(many, random_state=seed + n_points).as_matrix()
    y = 1.7 * np.einsum("bni,bij->bnj", x, rot) + 0.05 * rng.standard_normal(x.shape) + np.array([3.0, -2.0, 7.0])
    if n_points >= 4:
        s = covariance_singular_values(x, y)
        keep = s[:, 1] + s[:, 2] >= 0.1
        assert keep.sum() >= items, (n_points, keep.sum())
        x, y = x[keep], y[keep]
    x, y = np.ascontiguousarray(x[:items]), np.ascontiguousarray(y[:items])
    x.setflags(write=False), y.setflags(write=False)
    return x, y


def covariance_singular_values(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    x0, y0 = x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)
    x0 = x0 / np.linalg.norm(x0, axis=(1, 2), keepdims=True)
    y0 = y0 / np.linalg.norm(y0, axis=(1, 2), keepdims=True)
    return np.linalg.svd(np.einsum("bni,bnj->bij", x0, y0), compute_uv=False)


def torch_procrustes(x: np.ndarray, y: np.ndarray):
    from dad_3dheads_amd import evaluation

    return tuple(t.numpy() for t in evaluation.procrustes(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))))


def aligned(x_or_y: np.ndarray, b: np.ndarray, t: np.ndarray, c: np.ndarray) -> np.ndarray:
    return b[:, None, None] * np.einsum("bni,bij->bnj", x_or_y, t) + c[:, None]


def assert_procrustes(got, x: np.ndarray, y: np.ndarray, ref=None, what: str = "") -> None:
    """`got` = (b, T, c, flags) against `ref` = (b, T, c) (None: `evaluation.procrustes`): T within 1e-12 absolute, b and c within
    1e-12 relative -- c relative to its largest component, since a component of c = mu_x - b mu_y T is a difference of numbers of
    that size and has no relative accuracy of its own. With fewer than four points the covariance is singular and T is not
    unique: then T^T T = I within 1e-12, everything finite, b as above (the singular values are unique), and the aligned points
    b y T + c, which every valid T agrees on, within 1e-12 of their size."""
    b, t, c, flags = got
    rb, rt, rc = torch_procrustes(x, y) if ref is None else ref
    assert np.all(flags == 0), (what, flags)
    assert np.isfinite(b).all() and np.isfinite(t).all() and np.isfinite(c).all(), what
    assert np.abs(b - rb).max() <= 1e-12 * np.abs(rb).min(), (what, np.abs(b - rb).max())
    assert np.abs(np.einsum("bji,bjk->bik", t, t) - np.eye(3)).max() <= 1e-12, what
    if x.shape[1] >= 4:
        assert np.abs(t - rt).max() <= 1e-12, (what, np.abs(t - rt).max())
        assert np.all(np.abs(c - rc).max(1) <= 1e-12 * np.abs(rc).max(1)), (what, (np.abs(c - rc).max(1) / np.abs(rc).max(1)).max())
    else:
        a, ra = aligned(y, b, t, c), aligned(y, rb, rt, rc)
        assert np.abs(a - ra).max() <= 1e-12 * np.abs(ra).max(), (what, np.abs(a - ra).max())
