"""Float64 restatement of the training-objective terms (csrc/train_objective.hip) that the parity bars are measured against,
and the seeded inputs the golden generator and the tests share. NumPy only; test infrastructure, not product code."""
from __future__ import annotations

import numpy as np

EPS = 1e-6
CRITERIA = ("l1", "l2", "smooth_l1")


# ---- seeded inputs ---------------------------------------------------------------------------------------------------
def iou_inputs(seed: int, b: int, c: int, h: int, w: int):
    """(logits fp32 [B,C,H,W], target uint8 [B,C,H,W]): gaussian-ish blobs as targets, logits that roughly follow them.
    Channel (0,0) has saturated logits (+-60), channel (0,1) an all-zero target."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0, h, (b, c, 1, 1)), rng.uniform(0, w, (b, c, 1, 1))
    sig = rng.uniform(1.5, 4.0, (b, c, 1, 1))
    blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig ** 2))
    target = np.uint8(255.0 * blob.astype(np.float32))
    logits = (8.0 * blob - 4.0 + rng.normal(0, 1.5, (b, c, h, w))).astype(np.float32)
    logits[0, 0] = np.where(rng.random((h, w)) < 0.5, -60.0, 60.0).astype(np.float32)
    if c > 1:
        target[0, 1] = 0
    return logits, target


def visibility_inputs(seed: int, b: int, n: int):
    """pred, pred_presence, target, target_presence (fp32); one NaN prediction under presence 0."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0, 1, (b, n, 2)).astype(np.float32)
    pred = (target + rng.normal(0, 0.6, (b, n, 2))).astype(np.float32)
    presence = (rng.random((b, n)) < 0.8).astype(np.float32)
    presence[0, 0] = 0.0
    pred[0, 0, 1] = np.nan
    return pred, presence.copy(), target, presence.copy()


def keypoint_inputs(seed: int, b: int, n: int, dims: int, spread: float):
    """pred, target [B,N,dims] fp32, presence [B,N] fp32 and integer bboxes [B,4]."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.2, 0.8, (b, n, dims)).astype(np.float32)
    scale = rng.uniform(0.2, 2.0, (b, 1, 1)) * spread
    pred = (target + scale * rng.normal(0, 1, (b, n, dims))).astype(np.float32)
    presence = (rng.random((b, n)) < 0.85).astype(np.float32)
    bbox = np.stack([rng.integers(0, 50, b), rng.integers(0, 50, b), rng.integers(120, 250, b), rng.integers(120, 250, b)], 1)
    return pred, target, presence, bbox.astype(np.int64)


# ---- the terms, float64 from the fp32 inputs -------------------------------------------------------------------------
def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def target64(t):
    t = np.asarray(t)
    return t.astype(np.float32) / np.float32(255.0) if t.dtype == np.uint8 else t.astype(np.float32)


def iou_channels(s, t):
    """per-channel (N, D, IoU) of probabilities s and targets t, [B,C,...] -> [B,C]."""
    s = np.asarray(s, dtype=np.float64)
    t = np.asarray(target64(t), dtype=np.float64)
    ax = tuple(range(2, s.ndim))
    st, tt, ss = (t * s).sum(ax), (t * t).sum(ax), (s * s).sum(ax)
    n, d = st + EPS, tt + ss - st + EPS
    return n, d, n / d


def iou_loss(logits, target):
    """(loss, per-channel IoU [B,C], dL/dlogits) of IoULoss in float64."""
    s = sigmoid64(logits)
    n, d, iou = iou_channels(s, target)
    t = np.asarray(target64(target), dtype=np.float64)
    bc = iou.size
    k, nn_, dd = (-1.0 / (bc * d * d))[..., None, None], n[..., None, None], d[..., None, None]
    grad = k * (t * dd - nn_ * (2 * s - t)) * s * (1 - s)
    return 1.0 - iou.mean(), iou, grad


def soft_iou(probs, target):
    return iou_channels(probs, target)[2].mean()


def _crit(crit, d):
    ad = np.abs(d)
    if crit == "l1":
        return ad, np.sign(np.nan_to_num(d, nan=0.0))  # torch.sign(nan) = 0
    if crit == "l2":
        return d * d, 2 * d
    with np.errstate(invalid="ignore"):
        return np.where(ad < 1.0, 0.5 * d * d, ad - 0.5), np.where(d < -1.0, -1.0, np.where(d > 1.0, 1.0, d))


def visibility_loss(pred, pp, target, tp, crit):
    """(loss, dL/dpred) of LandmarksLossWVisibility in float64 (the fp32 products of the reference are exact: presences are 0/1)."""
    p = np.asarray(pred, np.float64) * np.asarray(pp, np.float64)[..., None]
    q = np.asarray(target, np.float64) * np.asarray(tp, np.float64)[..., None]
    val, slope = _crit(crit, p - q)
    m = p.size
    return val.sum() / m, slope / m * np.asarray(pp, np.float64)[..., None]


def normalize_to_cube(v):
    v = np.asarray(v, np.float64)
    v = v - v.min(1, keepdims=True)
    v = v - 0.5 * v.max(1, keepdims=True)
    return v / v.max(-1, keepdims=True).max(-2, keepdims=True)


def keypoint_errors(pred, target, bbox=None, index=None, presence=None, pred_scale=1.0, target_scale=1.0, cube=False):
    """(err [B], norm [B]) of metrics/keypoints.py in float64."""
    p, q = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    if presence is not None:
        pr = np.asarray(presence, np.float64)[..., None]
        p, q = p * pred_scale * pr, q * pr * target_scale
    else:
        p, q = p * pred_scale, q * target_scale
    if index is not None:
        p, q = p[:, index], q[:, index]
    if cube:
        p, q = normalize_to_cube(p), normalize_to_cube(q)
    err = np.sqrt(((p - q) ** 2).sum(-1)).mean(-1)
    norm = np.sqrt(np.asarray(bbox, np.float64)[:, 2] * np.asarray(bbox, np.float64)[:, 3]) if bbox is not None else np.full(err.shape, 2.0)
    return err, norm


def nme_and_rates(err, norm, thresholds=(0.05, 0.1)):
    return (err / norm).mean(), [float((err < t * norm).mean()) for t in thresholds]


# ---- the heatmap encode, restated from the host table and the floor-divide rule ---------------------------------------
def encode(keypoints, presence, size, stride, radius, form):
    """[B,C,2], [B,C] -> [B,C,S,S] in `form`, placing `coder.stamp_table` like draw_gaussian's clipped slices."""
    from dad_3dheads_amd.coder import floor_divide_f32, stamp_table

    table = stamp_table(radius, form)
    r = 1 if radius == "pointwise" else int(radius)
    kp = np.asarray(keypoints, np.float32)
    b, c = kp.shape[:2]
    out = np.zeros((b, c, size, size), dtype=table.dtype)
    centre = floor_divide_f32(kp, stride)
    for i in range(b):
        for j in range(c):
            if not presence[i, j]:
                continue
            fx, fy = centre[i, j]
            if not (np.isfinite(fx) and np.isfinite(fy)):
                raise ValueError("cannot convert float NaN to integer")
            if not (-r <= fx < size + r and -r <= fy < size + r):
                continue
            x, y = int(fx), int(fy)
            x0, x1, y0, y1 = max(x - r, 0), min(x + r + 1, size), max(y - r, 0), min(y + r + 1, size)
            out[i, j, y0:y1, x0:x1] = table[y0 - y + r: y1 - y + r, x0 - x + r: x1 - x + r]
    return out


def boundary_keypoints(size, stride, radius, seed, n_random=8):
    """[2,C,2] float32 keypoints and [2,C] presence: every boundary centre (-r-1, -r, -1, 0, S-1, S, S+r-1, S+r) on x and y,
    random points, huge finite coordinates, and NaN points with presence false."""
    r = 1 if radius == "pointwise" else int(radius)
    rng = np.random.default_rng(seed)
    edges = [-r - 1, -r, -1, 0, size - 1, size, size + r - 1, size + r]
    mid = size // 2
    cells = [(e, mid) for e in edges] + [(mid, e) for e in edges] + [(edges[0], edges[-1]), (edges[1], edges[6])]
    pts = [((cx + 0.25) * stride, (cy + 0.75) * stride) for cx, cy in cells]
    pts += [tuple(rng.uniform(-2 * stride, (size + 2) * stride, 2)) for _ in range(n_random)]
    pts += [(1e30, 5.0), (-3e29, -7e28), (np.nan, 3.0), (4.0, np.nan)]
    kp = np.asarray(pts, dtype=np.float32)
    presence = np.ones(len(pts), dtype=bool)
    presence[-2:] = False  # NaN points that are absent: no error in the reference, channel stays zero
    kp2 = np.stack([kp, rng.uniform(-stride, (size + 1) * stride, kp.shape).astype(np.float32)])
    pr2 = np.stack([presence, rng.random(len(pts)) < 0.7])
    return kp2, pr2
