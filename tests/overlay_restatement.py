"""The overlay stroke rules (include/dad3d.h) in plain numpy and Python integers, sequential: one primitive after
another, drawn into the image in place. The kernels of csrc/overlay.hip are held to this bit for bit. Nothing here is shared with
the package: `dad_3dheads_amd.overlay` is not imported.

A point table is float32 [P,2] (x, y); a coordinate is truncated toward zero. A primitive is skipped whole when one of its
coordinates is non-finite or truncates outside [-8192, 8192], or when it names a point outside the table.
"""
import math

import numpy as np

COORD_MAX = 8192


def truncate(v):
    """astype(int) of one coordinate, or None where the primitive is to be skipped."""
    v = float(v)
    if not math.isfinite(v):
        return None
    t = int(v)  # toward zero
    return t if -COORD_MAX <= t <= COORD_MAX else None


def point(points, i):
    if not 0 <= int(i) < len(points):
        return None
    x, y = truncate(points[int(i)][0]), truncate(points[int(i)][1])
    return None if x is None or y is None else (x, y)


def blend(image, x, y, color, a):
    """dst = (dst (256 - a) + colour a + 128) >> 8 on the pixel, where it lies in the image."""
    h, w = image.shape[:2]
    if 0 <= x < w and 0 <= y < h and a:
        for c in range(3):
            image[y, x, c] = (int(image[y, x, c]) * (256 - a) + int(color[c]) * a + 128) >> 8


def disc_mask(h, w, c, r):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    return (xs - c[0]) ** 2 + (ys - c[1]) ** 2 <= r * r


def window(image, lo, hi, grow):
    """The part of the image within `grow` pixels of the box lo .. hi, and its origin: a rule is a function of pixel - primitive, so
    it may be evaluated there alone."""
    h, w = image.shape[:2]
    x0, x1 = max(0, min(lo[0], hi[0]) - grow), min(w, max(lo[0], hi[0]) + grow + 1)
    y0, y1 = max(0, min(lo[1], hi[1]) - grow), min(h, max(lo[1], hi[1]) + grow + 1)
    return (image[y0:y1, x0:x1], x0, y0) if x0 < x1 and y0 < y1 else (None, 0, 0)


def draw_disc(image, c, r, color):
    sub, x0, y0 = window(image, c, c, r)
    if sub is not None:
        sub[disc_mask(sub.shape[0], sub.shape[1], (c[0] - x0, c[1] - y0), r)] = color


def solid_mask(h, w, p0, p1, t):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    l2 = dx * dx + dy * dy
    ux, uy, vx, vy = xs - p0[0], ys - p0[1], xs - p1[0], ys - p1[1]
    dot, cr = ux * dx + uy * dy, ux * dy - uy * dx
    body = (dot >= 0) & (dot <= l2) & (4 * cr * cr <= t * t * l2) & (l2 > 0)  # a zero-length segment leaves only the end tests
    return body | (4 * (ux * ux + uy * uy) <= t * t) | (4 * (vx * vx + vy * vy) <= t * t)


def draw_solid(image, p0, p1, t, color):
    sub, x0, y0 = window(image, p0, p1, t)  # nothing farther than t / 2 from the segment is inside
    if sub is not None:
        sub[solid_mask(sub.shape[0], sub.shape[1], (p0[0] - x0, p0[1] - y0), (p1[0] - x0, p1[1] - y0), t)] = color


def aa_steps(p0, p1):
    """int64 [2 (n + 1), 3] rows (x, y, a) in drawing order: for every step the pixel at `base` with 256 - frac, then its neighbour
    at base + 1 with frac. No pixel appears twice: the steps differ in the major coordinate, the two of a step in the minor one."""
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    x_major = abs(dx) >= abs(dy)
    d_major, d_minor = (dx, dy) if x_major else (dy, dx)
    m0, minor0 = (p0[0], p0[1]) if x_major else (p0[1], p0[0])
    n, sign = abs(d_major), (1 if d_major >= 0 else -1)
    i = np.arange(n + 1, dtype=np.int64)
    major = m0 + i * sign
    q = 256 * minor0 + ((2 * i * d_minor * 256 + n) // (2 * n) if n else 0 * i)  # numpy's // on int64 is floor division
    base, frac = q >> 8, q & 255  # >> on a negative int64 is arithmetic
    major = np.repeat(major, 2)
    minor = np.stack([base, base + 1], 1).reshape(-1)
    a = np.stack([256 - frac, frac], 1).reshape(-1)
    return np.stack([major, minor, a] if x_major else [minor, major, a], 1)


def draw_aa(image, p0, p1, color):
    h, w = image.shape[:2]
    x, y, a = aa_steps(p0, p1).T
    keep = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    x, y, a = x[keep], y[keep], a[keep, None]
    dst = image[y, x].astype(np.int64)  # distinct pixels: one vectorised blend equals the pixel-by-pixel walk
    image[y, x] = ((dst * (256 - a) + np.asarray(color, dtype=np.int64)[None] * a + 128) >> 8).astype(np.uint8)


def draw_segments(image, points, edges, color=None, colors=None, thickness=0):
    """Segment e = (points[edges[e][0]], points[edges[e][1]]) in ascending e; thickness 0 is anti-aliased. In place."""
    for e, (i0, i1) in enumerate(np.asarray(edges).reshape(-1, 2)):
        p0, p1 = point(points, i0), point(points, i1)
        if p0 is None or p1 is None:
            continue
        c = colors[e] if colors is not None else color
        if thickness == 0:
            draw_aa(image, p0, p1, c)
        else:
            draw_solid(image, p0, p1, thickness, c)
    return image


def draw_discs(image, points, radius, color, index=None):
    for i in (range(len(points)) if index is None else index):
        c = point(points, i)
        if c is not None:
            draw_disc(image, c, radius, color)
    return image


# -- the host side of draw_pose and calculate_rpy (model_training/model/flame.py:239-264, demo_utils.py:68-94), line by line --------
def limit_angle(angle, pi=180.0):
    if angle < -pi:
        k = -2 * (int(angle / pi) // 2)
        angle = angle + k * pi
    if angle > pi:
        k = 2 * ((int(angle / pi) + 1) // 2)
        angle = angle - k * pi
    return angle


def rot_mat_from_6dof(v):
    """model_training/model/utils.py:92-101 for one row, float32 through torch like the reference."""
    import torch
    import torch.nn.functional as F

    v = torch.as_tensor(np.asarray(v, dtype=np.float32)).view(-1, 6)
    vx, vy = v[..., :3].clone(), v[..., 3:].clone()
    b1 = F.normalize(vx, dim=-1)
    b3 = F.normalize(torch.cross(b1, vy, dim=-1), dim=-1)
    b2 = -torch.cross(b1, b3, dim=-1)
    return torch.stack((b1, b2, b3), dim=-1)


def calculate_rpy(rotation_6dof):
    from scipy.spatial.transform import Rotation

    rot_mat = rot_mat_from_6dof(rotation_6dof).numpy()[0]
    angle = Rotation.from_matrix(np.transpose(rot_mat)).as_euler("xyz", degrees=True)
    return tuple(map(limit_angle, [angle[2], angle[0] - 180, angle[1]]))  # roll, pitch, yaw


def pose_axes(rpy, h, w):
    """demo_utils.py:73-92: the centre and the three end points, int() truncated."""
    tdx, tdy = w // 2, h // 2
    roll, pitch, yaw = rpy[0] * np.pi / 180, rpy[1] * np.pi / 180, -(rpy[2] * np.pi / 180)
    size = h // 10
    x1 = size * (np.cos(yaw) * np.cos(roll)) + tdx
    y1 = size * (np.cos(pitch) * np.sin(roll) + np.cos(roll) * np.sin(pitch) * np.sin(yaw)) + tdy
    x2 = size * (-np.cos(yaw) * np.sin(roll)) + tdx
    y2 = size * (np.cos(pitch) * np.cos(roll) - np.sin(pitch) * np.sin(yaw) * np.sin(roll)) + tdy
    x3 = size * (np.sin(yaw)) + tdx
    y3 = size * (-np.cos(yaw) * np.sin(pitch)) + tdy
    return (int(tdx), int(tdy)), [(int(x1), int(y1)), (int(x2), int(y2)), (int(x3), int(y3))]


def arrow_tips(p1, p2):
    """The two tip ends of an arrow from p1 to p2: length 0.1 |p1 - p2|, at atan2(p1 - p2) +- pi / 4, rounded half to even."""
    tip = 0.1 * math.hypot(p1[0] - p2[0], p1[1] - p2[1])
    angle = math.atan2(p1[1] - p2[1], p1[0] - p2[0])
    return [(round(p2[0] + tip * math.cos(angle + s * math.pi / 4)), round(p2[1] + tip * math.sin(angle + s * math.pi / 4)))
            for s in (1, -1)]


POSE_COLORS = ((0, 0, 255), (0, 255, 0), (255, 0, 0))


def draw_pose(image, rpy):
    h, w = image.shape[:2]
    t = int(h * 0.005)
    centre, ends = pose_axes(rpy, h, w)
    for end, color in zip(ends, POSE_COLORS):
        tips = arrow_tips(centre, end)
        for p0, p1 in ((centre, end), (end, tips[0]), (end, tips[1])):
            draw_solid(image, p0, p1, t, color)
    return image
