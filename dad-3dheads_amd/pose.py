"""Head pose where the params lie: the rotation matrix of `rot_mat_from_6dof`, (roll, pitch, yaw) as the reference's `calculate_rpy`
gives them (model_training/model/flame.py:254-264), the arrows of `draw_pose`, and the scorer's Procrustes alignment, as the two
kernels of csrc/head_pose.hip. Nothing here waits for the device.

The angles follow scipy's `Rotation.from_matrix(M).as_euler("xyz", degrees=True)` step for step -- orthogonal polar factor,
quaternion by the largest of (m00, m11, m22, trace), half-angle formulas with the lock rule -- because the textbook atan2 of
matrix entries differs from it by up to 1.4e-4 degrees on a float32 matrix. `rpy_rows` is the same rule in numpy, for host values
and as the statement the tests hold the kernels to.

`rotation` is `rot_mat_from_6dof` as the reference computes it. Which convention the benchmark's `rotation_matrix` field wants
relative to `rot_180 @ model_view` cannot be checked without the dataset and a trained checkpoint; a submission driver is not part
of this module."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .flame import _SLICE_ORDER, FLAME_CONSTS

N_PARAMS = sum(FLAME_CONSTS.values())
ROTATION_OFFSET = sum(FLAME_CONSTS[k] for k in _SLICE_ORDER[:_SLICE_ORDER.index("rotation")])  # 403: shape, expression, jaw in front
N_POSE_POINTS = 10
LOCK_EPS = 1e-7          # scipy's `eps` of _get_angles, radians
MIN_SINGULAR = 1e-6      # below it the polar factor of a pose matrix counts as undefined (DAD3D_POSE_FLAG_DEGENERATE)
_WANT = ("rotation", "rpy", "points", "flags")


class HeadPose(NamedTuple):
    """What `head_pose` returns; a field that was not asked for is None."""
    rotation: Optional[Tensor]  # float32 [n,3,3]: columns b1 b2 b3
    rpy: Optional[Tensor]       # float64 [n,3]: roll, pitch, yaw in degrees
    points: Optional[Tensor]    # float32 [n,10,2]: the point table `overlay._launch_segments` takes
    flags: Tensor               # int32 [n]: _lib.POSE_FLAG_*


def _rows(t: Tensor) -> Tuple[Tensor, int]:
    """`params [n,413]` or `rot6 [n,6]` (or one row of either) -> (a float32 tensor with a unit last stride, the rotation's offset)."""
    if t.ndim == 1:
        t = t[None]
    if t.ndim != 2 or t.shape[1] not in (6, N_PARAMS):
        raise ValueError(f"params_or_rot6: expected [n,{N_PARAMS}] or [n,6], got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < 0) or t.shape[0] <= 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (0 if t.shape[1] == 6 else ROTATION_OFFSET)


def head_pose(params_or_rot6: Tensor, frames: Any = None, image_index: Optional[Tensor] = None, size: Optional[Tuple[int, int]] = None,
              want: Sequence[str] = ("rotation", "rpy")) -> HeadPose:
    """`dad3d_head_pose` on the current stream: one launch, everything stays on the device, nothing waits.

    `params_or_rot6`: a CUDA tensor `[n,413]` (a strided view of one works where it lies) or the bare 6-D rotations `[n,6]`.
    `want`: which of "rotation", "rpy", "points" to compute ("flags" always are). The points need the frame of every head: `size`
    = one `(h, w)` for all, or `frames` with a CUDA `image_index [n]`. `frames`: the int64 device table `[M,4]` {address, h, w, row
    stride} of `dad3d_preprocess_boxes`, or a list of frames (tensors, arrays or `(h, w)` pairs: only their sizes are read).
    A NaN / Inf row, or one whose polar factor is undefined, gets its flag, NaN angles and all ten points at the frame's centre;
    a head whose index names no frame gets `POSE_FLAG_INDEX` and zero points."""
    if not isinstance(params_or_rot6, Tensor) or not params_or_rot6.is_cuda:
        raise ValueError("params_or_rot6: expected a CUDA tensor (head_pose runs on the GPU; rpy_rows is the host rule)")
    unknown = [w for w in want if w not in _WANT]
    if unknown:
        raise ValueError(f"want: {unknown} not among {_WANT}")
    rows, offset = _rows(params_or_rot6)
    dev, n = rows.device, rows.shape[0]
    table = index = None
    h = w = 0
    if "points" in want:
        if (frames is None) == (size is None):
            raise ValueError("points: give either size=(h, w) or frames= with image_index=")
        if size is not None:
            h, w = int(size[0]), int(size[1])
            if h < 1 or w < 1:
                raise ValueError(f"size: expected positive (h, w), got {size!r}")
        else:
            if not isinstance(image_index, Tensor) or not image_index.is_cuda or tuple(image_index.shape) != (n,) or image_index.is_floating_point():
                raise ValueError(f"image_index: frames need a CUDA integer tensor [{n}]")
            index = image_index.to(dev, torch.int32).contiguous()
            if isinstance(frames, Tensor) and frames.dtype == torch.int64 and frames.ndim == 2 and frames.shape[1] == 4:
                table = frames.to(dev).contiguous()
            else:  # sizes only: a placeholder address, which the kernel never reads
                table = torch.tensor([[1, *(int(s) for s in (f.shape[:2] if hasattr(f, "shape") else f[:2])), 0] for f in frames],
                                     dtype=torch.int64).reshape(-1, 4).to(dev)
    out = {"rotation": torch.empty((n, 3, 3), dtype=torch.float32, device=dev) if "rotation" in want else None,
           "rpy": torch.empty((n, 3), dtype=torch.float64, device=dev) if "rpy" in want else None,
           "points": torch.empty((n, N_POSE_POINTS, 2), dtype=torch.float32, device=dev) if "points" in want else None}
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    if n:
        _lib.check(_lib.load().dad3d_head_pose(rows.data_ptr(), n, rows.stride(0) if n > 1 else rows.shape[1], offset, ptr(table),
                                               0 if table is None else table.shape[0], ptr(index), h, w, ptr(out["rotation"]), ptr(out["rpy"]),
                                               ptr(out["points"]), flags.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream))
    return HeadPose(out["rotation"], out["rpy"], out["points"], flags)


def head_pose_host(params_or_rot6, frame_sizes=None, image_index=None, size: Optional[Tuple[int, int]] = None,
                   want: Sequence[str] = _WANT):
    """`dad3d_head_pose_host`: the kernel's routine on the CPU, numpy in and out, no GPU needed. `frame_sizes`: `[(h, w), ..]` with
    `image_index [n]`, or `size` for all rows. -> HeadPose of numpy arrays."""
    rows = np.ascontiguousarray(np.asarray(params_or_rot6, dtype=np.float32))
    if rows.ndim == 1:
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] not in (6, N_PARAMS):
        raise ValueError(f"params_or_rot6: expected [n,{N_PARAMS}] or [n,6], got shape {rows.shape}")
    n = rows.shape[0]
    offset = 0 if rows.shape[1] == 6 else ROTATION_OFFSET
    table = index = None
    h, w = (0, 0) if size is None else (int(size[0]), int(size[1]))
    if frame_sizes is not None:
        table = np.ascontiguousarray([[1, int(s[0]), int(s[1]), 0] for s in frame_sizes], dtype=np.int64).reshape(-1, 4)
        index = np.ascontiguousarray(np.asarray(image_index).reshape(-1), dtype=np.int32)
        if index.shape[0] != n:
            raise ValueError(f"image_index: {index.shape[0]} entries for {n} rows")
    out = {"rotation": np.empty((n, 3, 3), np.float32) if "rotation" in want else None,
           "rpy": np.empty((n, 3), np.float64) if "rpy" in want else None,
           "points": np.empty((n, N_POSE_POINTS, 2), np.float32) if "points" in want else None}
    flags = np.empty((n,), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.load().dad3d_head_pose_host(ptr(rows), n, rows.shape[1], offset, ptr(table), 0 if table is None else table.shape[0], ptr(index),
                                                h, w, ptr(out["rotation"]), ptr(out["rpy"]), ptr(out["points"]), ptr(flags)))
    return HeadPose(out["rotation"], out["rpy"], out["points"], flags)


# -- the rule in numpy -----------------------------------------------------------------------------------------------------------------
def rotation_rows(rot6) -> np.ndarray:
    """`rot_mat_from_6dof` in float32 as the device computes it: sqrt of the left-to-right sum of squares, the clamp at 1e-12, three
    divisions, the two crosses. `[n,6]` -> float32 `[n,3,3]`, columns b1 b2 b3."""
    v = np.asarray(rot6, dtype=np.float32).reshape(-1, 6)
    f = np.float32

    def normalize(a):
        n = np.maximum(np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]), f(1e-12))
        return a / n[:, None]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    with np.errstate(all="ignore"):
        b1 = normalize(v[:, :3])
        b3 = normalize(cross(b1, v[:, 3:]))
        b2 = -cross(b1, b3)
    return np.stack([b1, b2, b3], axis=-1).astype(np.float32)


def limit_angle(angle: float, pi: float = 180.0) -> float:
    """model_training/model/flame.py:239-251, degrees."""
    if angle < -pi:
        k = -2 * (int(angle / pi) // 2)
        angle = angle + k * pi
    if angle > pi:
        k = 2 * ((int(angle / pi) + 1) // 2)
        angle = angle - k * pi
    return angle


def quat_from_matrix(m: np.ndarray) -> np.ndarray:
    """scipy's `from_matrix` behind its polar factor: (x, y, z, w) by the largest of m00, m11, m22, trace; normalised."""
    d = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
    choice = int(np.argmax(d))
    q = [0.0] * 4
    if choice != 3:
        i = choice
        j, k = (i + 1) % 3, (i + 2) % 3
        q[i] = 1.0 - d[3] + 2.0 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    else:
        q = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + d[3]]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([c / n for c in q], dtype=np.float64)


def euler_xyz_from_quat(q) -> Tuple[Tuple[float, float, float], bool]:
    """scipy's `as_euler("xyz")` in radians (Bernardes and Viollet's half-angle formulas) -> (angles, lock branch taken)."""
    a, b, c, d = q[3] - q[1], q[0] + q[2], q[1] + q[3], q[2] - q[0]
    a1 = 2.0 * math.atan2(math.hypot(c, d), math.hypot(a, b))
    lock = 1 if abs(a1) <= LOCK_EPS else 2 if abs(a1 - math.pi) <= LOCK_EPS else 0
    half_sum, half_diff = math.atan2(b, a), math.atan2(d, c)
    if lock == 0:
        a0, a2 = half_sum - half_diff, half_sum + half_diff
    else:
        a2 = 0.0
        a0 = 2.0 * half_sum if lock == 1 else 2.0 * half_diff * -1.0
    a1 -= math.pi / 2.0
    wrap = lambda x: x + 2.0 * math.pi if x < -math.pi else x - 2.0 * math.pi if x > math.pi else x  # noqa: E731
    return (wrap(a0), wrap(a1), wrap(a2)), lock != 0


def euler_rows(matrices) -> Tuple[np.ndarray, np.ndarray]:
    """`Rotation.from_matrix(M).as_euler("xyz", degrees=True)` restated, per matrix: `[n,3,3]` -> (degrees float64 `[n,3]`, flags
    int32 `[n]`). A matrix scipy would refuse (non-finite, singular, determinant <= 0) gets NaN angles and its flag."""
    ms = np.asarray(matrices).reshape(-1, 3, 3)
    out = np.full((ms.shape[0], 3), np.nan)
    flags = np.zeros(ms.shape[0], np.int32)
    for n, m in enumerate(ms):
        m = m.astype(np.float64)
        if not np.isfinite(m).all():
            flags[n] = _lib.POSE_FLAG_NONFINITE
            continue
        u, s, vt = np.linalg.svd(m)
        if s[2] < MIN_SINGULAR or not np.linalg.det(m) > 0.0:
            flags[n] = _lib.POSE_FLAG_DEGENERATE
            continue
        angles, lock = euler_xyz_from_quat(quat_from_matrix(u @ vt))
        out[n] = [x * (180.0 / math.pi) for x in angles]
        flags[n] = _lib.POSE_FLAG_GIMBAL if lock else 0
    return out, flags


def rpy_rows(rot6) -> Tuple[np.ndarray, np.ndarray]:
    """(roll, pitch, yaw) in degrees of 6-D rotations `[n,6]` by the device's rule, in numpy: float32 for the matrix, float64 behind
    it, `math` for the transcendental functions. -> (float64 `[n,3]`, flags int32 `[n]`)."""
    v = np.asarray(rot6, dtype=np.float32).reshape(-1, 6)
    angles, flags = euler_rows(np.transpose(rotation_rows(v), (0, 2, 1)))
    flags[~np.isfinite(v).all(1)] = _lib.POSE_FLAG_NONFINITE
    out = np.full_like(angles, np.nan)
    for n in np.flatnonzero(np.isfinite(angles).all(1) & np.isfinite(v).all(1)):
        a = angles[n]
        out[n] = [limit_angle(float(a[2])), limit_angle(float(a[0]) - 180.0), limit_angle(float(a[1]))]
    return out, flags


def arrow_points(rpy, h: int, w: int) -> np.ndarray:
    """The ten points of the three arrows (demo_utils.py:73-92, `overlay.pose_points`) for one (roll, pitch, yaw) in degrees, float64
    `[10,2]` BEFORE truncation and rounding, so a caller can see how close a coordinate lies to an edge: the centre, the three ends,
    then the six tip ends computed from the truncated ends. Non-finite angles: the centre ten times."""
    tdx, tdy, size = w // 2, h // 2, h // 10
    if not np.isfinite(np.asarray(rpy, dtype=np.float64)).all():
        return np.tile(np.array([[tdx, tdy]], dtype=np.float64), (10, 1))
    roll, pitch, yaw = rpy[0] * math.pi / 180, rpy[1] * math.pi / 180, -(rpy[2] * math.pi / 180)
    ends = [(size * (math.cos(yaw) * math.cos(roll)) + tdx,
             size * (math.cos(pitch) * math.sin(roll) + math.cos(roll) * math.sin(pitch) * math.sin(yaw)) + tdy),
            (size * (-math.cos(yaw) * math.sin(roll)) + tdx,
             size * (math.cos(pitch) * math.cos(roll) - math.sin(pitch) * math.sin(yaw) * math.sin(roll)) + tdy),
            (size * math.sin(yaw) + tdx, size * (-math.cos(yaw) * math.sin(pitch)) + tdy)]
    tips = []
    for ex, ey in ends:
        x, y = int(ex), int(ey)
        tip = 0.1 * math.hypot(tdx - x, tdy - y)
        angle = math.atan2(tdy - y, tdx - x)
        for s in (1, -1):
            tips.append((x + tip * math.cos(angle + s * math.pi / 4), y + tip * math.sin(angle + s * math.pi / 4)))
    return np.array([(tdx, tdy)] + ends + tips, dtype=np.float64)


def snap_points(raw: np.ndarray) -> np.ndarray:
    """`arrow_points` -> the table the kernel writes: ends truncated toward zero, tips rounded half to even, float32."""
    out = np.array(raw, dtype=np.float64)
    out[..., 1:4, :] = np.trunc(out[..., 1:4, :])
    out[..., 4:, :] = np.rint(out[..., 4:, :])
    return out.astype(np.float32)


# -- Procrustes ------------------------------------------------------------------------------------------------------------------------
def procrustes_batch(x: Tensor, y: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`evaluation.procrustes` on the device (`dad3d_procrustes`, one wave per item): X, Y `[B,n,3]` CUDA tensors -> (b `[B]`, T
    `[B,3,3]`, c `[B,3]` float64, flags int32 `[B]`) such that b * Y . T + c best fits X; T may be a reflection. An item whose centred
    norm is 0 or not finite gets `POSE_FLAG_DEGENERATE` and NaN. One launch, no wait; an item's bits do not depend on the batch."""
    if not (isinstance(x, Tensor) and isinstance(y, Tensor) and x.is_cuda and y.device == x.device):
        raise ValueError("procrustes_batch: expected two CUDA tensors on one device (evaluation.procrustes is the host rule)")
    if x.ndim != 3 or x.shape[2] != 3 or x.shape != y.shape or x.shape[1] < 1:
        raise ValueError(f"procrustes_batch: expected X and Y of one shape [B,n,3], got {tuple(x.shape)} and {tuple(y.shape)}")
    x, y = x.to(torch.float64).contiguous(), y.to(torch.float64).contiguous()
    dev, bsz = x.device, x.shape[0]
    b = torch.empty((bsz,), dtype=torch.float64, device=dev)
    t = torch.empty((bsz, 3, 3), dtype=torch.float64, device=dev)
    c = torch.empty((bsz, 3), dtype=torch.float64, device=dev)
    flags = torch.empty((bsz,), dtype=torch.int32, device=dev)
    if bsz:
        _lib.check(_lib.load().dad3d_procrustes(x.data_ptr(), y.data_ptr(), bsz, x.shape[1], b.data_ptr(), t.data_ptr(), c.data_ptr(),
                                                flags.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream))
    return b, t, c, flags


def procrustes_host(x, y):
    """`dad3d_procrustes_host`: the kernel's routine on the CPU, numpy `[B,n,3]` in, (b, T, c, flags) out. No GPU needed."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if x.ndim != 3 or x.shape[2] != 3 or x.shape != y.shape or x.shape[1] < 1:
        raise ValueError(f"procrustes_host: expected X and Y of one shape [B,n,3], got {x.shape} and {y.shape}")
    bsz = x.shape[0]
    b, t, c = np.empty((bsz,), np.float64), np.empty((bsz, 3, 3), np.float64), np.empty((bsz, 3), np.float64)
    flags = np.empty((bsz,), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _lib.check(_lib.load().dad3d_procrustes_host(ptr(x), ptr(y), bsz, x.shape[1], ptr(b), ptr(t), ptr(c), ptr(flags)))
    return b, t, c, flags
