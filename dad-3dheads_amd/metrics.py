"""The training step's metrics (`model_training/metrics/iou.py`, `metrics/keypoints.py`, the metric block of
`train/flame_lightning_model.py:_step_fn`) on the HIP kernels of csrc/train_objective.hip.

The metric classes keep torchmetrics' surface with `compute_on_step=True`: `metric(...)` returns the batch value and adds it
to the running state; `compute()` returns the running value; `reset()` clears it. The states are device tensors that the
kernels add into, so no step waits for the device. `states` exposes them by their reference names for a caller that
all-reduces them across ranks (sum); that sync is not done here.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .heatmap_points import heatmap_peaks
from .losses import _f32, heatmap_iou_terms

__all__ = ["soft_iou", "keypoints_nme", "percentage_of_errors_below_IOD", "keypoint_errors", "SoftIoUMetric", "FailureRate",
           "KeypointsNME", "StepMetrics"]

# model_training/data/config.py keys
OUTPUT_LANDMARKS_HEATMAP, TARGET_LANDMARKS_HEATMAP = "OUTPUT_LANDMARKS_HEATMAP", "TARGET_LANDMARKS_HEATMAP"
OUTPUT_2D_LANDMARKS, TARGET_2D_LANDMARKS = "OUTPUT_2D_LANDMARKS", "TARGET_2D_LANDMARKS"
TARGET_2D_LANDMARKS_PRESENCE, TARGET_2D_FULL_LANDMARKS = "TARGET_2D_LANDMARKS_PRESENCE", "TARGET_2D_FULL_LANDMARKS"
OUTPUT_3DMM_PARAMS, TARGET_3D_MODEL_VERTICES, INPUT_BBOX_KEY = "OUTPUT_3DMM_PARAMS", "TARGET_3D_MODEL_VERTICES", "INPUT_BBOX_KEY"


def soft_iou(output: Tensor, target: Tensor, eps: float = 1e-6) -> Tensor:
    """metrics/iou.py:15-31: mean over [B,C] of the soft IoU of probabilities `output` and `target`."""
    if eps != 1e-6:
        raise ValueError("the kernel's eps is the reference's 1e-6")
    return heatmap_iou_terms(output, target, sigmoid=False)[4][1]


def keypoint_errors(pred: Tensor, target: Tensor, bbox: Optional[Tensor] = None, *, index: Optional[Tensor] = None,
                    presence: Optional[Tensor] = None, pred_scale: float = 1.0, target_scale: float = 1.0, cube: bool = False,
                    thresholds: Sequence[float] = (), below: bool = True, accum: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One launch of dad3d_keypoint_errors: (out [1 + T] = (NME, fraction below thr_k ...), err [B,2] float64 = (err, norm)).
    pred / target [B,V,D]; index [n] int into V (the subset both are gathered to); presence [B,V] multiplies both (after
    `pred_scale` on pred, before `target_scale` on target, like _step_fn); cube: normalize_to_cube both subsets."""
    from . import _lib

    p, t = _f32(pred, "the predicted keypoints"), _f32(target, "the target keypoints")
    if p.ndim != 3 or p.shape != t.shape or p.shape[2] not in (2, 3):
        raise ValueError(f"expected two [B,V,2|3] keypoint tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    b, v, d = p.shape
    dev = p.device
    idx = None
    if index is not None:
        idx_np = np.asarray(index.cpu() if torch.is_tensor(index) else index, dtype=np.int64).reshape(-1)
        if idx_np.size and (idx_np.min() < -v or idx_np.max() >= v):
            raise IndexError(f"keypoint index out of range for {v} points")
        idx = torch.from_numpy(np.where(idx_np < 0, idx_np + v, idx_np).astype(np.int32)).to(dev)
    n = v if idx is None else idx.numel()
    pres = None if presence is None else _f32(presence, "the presence").reshape(b, v)
    bb = None
    if bbox is not None:
        if bbox.is_floating_point():
            raise TypeError("the bbox must be an integer tensor [B,4] (x, y, w, h)")
        bb = bbox.detach().to(dev, torch.int32).reshape(b, 4).contiguous()
    thr = [float(x) for x in thresholds]
    out = torch.empty(1 + len(thr), dtype=torch.float32, device=dev)
    err = torch.empty((b, 2), dtype=torch.float64, device=dev)
    thr_c = (C.c_double * max(1, len(thr)))(*thr)  # a HOST array: copied into the launch arguments
    _lib.check(_lib.load().dad3d_keypoint_errors(
        p.data_ptr(), t.data_ptr(), b, v, d, None if idx is None else idx.data_ptr(), n, None if pres is None else pres.data_ptr(),
        float(pred_scale), float(target_scale), int(cube), None if bb is None else bb.data_ptr(), thr_c, len(thr), int(below),
        err.data_ptr(), out.data_ptr(), None if accum is None else accum.data_ptr(), dev.index or 0,
        torch.cuda.current_stream(dev).cuda_stream))
    return out, err


def keypoints_nme(output_kp: Tensor, target_kp: Tensor, bbox: Tensor = None, reduce: str = "mean") -> Tensor:
    """metrics/keypoints.py:19-35."""
    out, err = keypoint_errors(output_kp, target_kp, bbox)
    if reduce == "mean":
        return out[0]
    return (err[:, 0] / err[:, 1]).to(torch.float32)


def percentage_of_errors_below_IOD(output_kp: Tensor, target_kp: Tensor, bbox: Tensor = None, threshold: float = 0.05,
                                   below: bool = True) -> Tensor:
    """metrics/keypoints.py:38-53."""
    return keypoint_errors(output_kp, target_kp, bbox, thresholds=(threshold,), below=below)[0][1]


class _Metric:
    """torchmetrics.Metric with compute_on_step=True, restated: a (value, total) pair of device float32 states, which the
    kernels add into (`_acc` may be a view into a buffer one launch fills for several metrics)."""

    _value_name = "value"

    def __init__(self, compute_on_step: bool = True, dist_sync_on_step: bool = False, process_group: Optional[Any] = None,
                 dist_sync_fn: Any = None) -> None:
        self.compute_on_step = compute_on_step
        self._acc: Optional[Tensor] = None

    def _state(self, device: torch.device) -> Tensor:
        if self._acc is None or self._acc.device != device:
            self._acc = torch.zeros(2, dtype=torch.float32, device=device)
        return self._acc

    @property
    def states(self) -> Dict[str, Tensor]:
        acc = self._acc if self._acc is not None else torch.zeros(2)
        return {self._value_name: acc[0], "total": acc[1]}

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()

    def __call__(self, *args, **kwargs) -> Optional[Tensor]:
        value = self._update(*args, **kwargs)
        return value if self.compute_on_step else None

    def update(self, *args, **kwargs) -> None:
        self._update(*args, **kwargs)

    forward = __call__


class SoftIoUMetric(_Metric):
    """metrics/iou.py:34-72 (ious, total)."""

    _value_name = "ious"

    def _update(self, preds: Tensor, target: Tensor) -> Tensor:
        return heatmap_iou_terms(preds, target, sigmoid=False, accum=self._state(preds.device))[4][1]

    def _update_logits(self, logits: Tensor, target: Tensor) -> Tensor:
        """update(sigmoid(logits), target) without materialising the sigmoid: the same per-channel values."""
        return heatmap_iou_terms(logits, target, sigmoid=True, accum=self._state(logits.device))[4][1]

    def compute(self) -> Tensor:
        acc = self._state(self._acc.device if self._acc is not None else torch.device("cuda"))
        return torch.mean(acc[0] / acc[1])


def _gts(gts: Mapping[str, Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
    return gts["keypoints"], gts["bboxes"] if "bboxes" in gts.keys() else None  # keypoints.py:11-16


class FailureRate(_Metric):
    """metrics/keypoints.py:56-104 (failure_rate, total)."""

    _value_name = "failure_rate"

    def __init__(self, compute_on_step: bool = True, dist_sync_on_step: bool = False, process_group: Optional[Any] = None,
                 dist_sync_fn: Any = None, threshold: float = 0.05, below: bool = True) -> None:
        super().__init__(compute_on_step, dist_sync_on_step, process_group, dist_sync_fn)
        self.threshold, self.below = threshold, below
        self._buf: Optional[Tensor] = None

    def _update(self, pred_keypoints: Tensor, gts: Mapping[str, Tensor]) -> Tensor:
        kp, bbox = _gts(gts)
        dev = pred_keypoints.device
        if self._buf is None or self._buf.device != dev:
            self._buf = torch.zeros(4, dtype=torch.float32, device=dev)  # (nme, total) slots the kernel also fills, then ours
            self._acc = self._buf[2:]
        return keypoint_errors(pred_keypoints, kp, bbox, thresholds=(self.threshold,), below=self.below, accum=self._buf)[0][1]

    def compute(self) -> Tensor:
        return self._acc[0] / self._acc[1]


class KeypointsNME(_Metric):
    """metrics/keypoints.py:107-151 (nme, total); `compute` is weight * nme / total."""

    _value_name = "nme"

    def __init__(self, compute_on_step: bool = True, dist_sync_on_step: bool = False, process_group: Optional[Any] = None,
                 dist_sync_fn: Any = None, weight: int = 100) -> None:
        super().__init__(compute_on_step, dist_sync_on_step, process_group, dist_sync_fn)
        self.weight = weight

    def _update(self, pred_keypoints: Tensor, gts: Mapping[str, Tensor]) -> Tensor:
        kp, bbox = _gts(gts)
        return self.weight * keypoint_errors(pred_keypoints, kp, bbox, accum=self._state(pred_keypoints.device))[0][0]

    def compute(self) -> Tensor:
        return self.weight * (self._acc[0] / self._acc[1])


class _KeypointGroup:
    """fr_005, fr_01 and nme of one branch from ONE launch: the three metrics' states are views into one buffer."""

    def __init__(self, prefix: str) -> None:
        self.names = (f"{prefix}fr_{{}}_005", f"{prefix}fr_{{}}_01", f"{prefix}nme_{{}}")
        self.fr005, self.fr01, self.nme = FailureRate(threshold=0.05), FailureRate(threshold=0.1), KeypointsNME()
        self._buf: Optional[Tensor] = None

    def __call__(self, pred: Tensor, target: Tensor, bbox: Optional[Tensor], **kw) -> Tuple[Tensor, Tensor, Tensor]:
        dev = pred.device
        if self._buf is None or self._buf.device != dev:
            self._buf = torch.zeros(6, dtype=torch.float32, device=dev)
            self.nme._acc, self.fr005._acc, self.fr01._acc = self._buf[0:2], self._buf[2:4], self._buf[4:6]
        out, _ = keypoint_errors(pred, target, bbox, thresholds=(0.05, 0.1), accum=self._buf, **kw)
        return out[1], out[2], self.nme.weight * out[0]

    def reset(self) -> None:
        if self._buf is not None:
            self._buf.zero_()


class StepMetrics:
    """The metric block of `_step_fn` (train/flame_lightning_model.py:305-357) in one call: returns {name: batch value} with
    the reference's log names (heatmap_iou, fr_2d_005, fr_2d_01, nme_2d, reproject_*, fr_3d_005, fr_3d_01, nme_3d) and
    accumulates every metric's state. `flame_indices` maps region names to vertex indices ("face" is used)."""

    def __init__(self, head_mesh, flame_indices: Mapping[str, Any], img_size: int, stride: int = 2) -> None:
        self.head_mesh = head_mesh
        self.stride = stride  # config["train"].get("stride", 2): the heatmap's pixel pitch in the image
        self.face = np.asarray(flame_indices["face"], dtype=np.int64)
        self.img_size = img_size
        self.iou_metric = SoftIoUMetric()
        self.metrics_2d, self.metrics_reprojection, self.metrics_3d = _KeypointGroup(""), _KeypointGroup("reproject_"), _KeypointGroup("")

    def reset(self) -> None:
        self.iou_metric.reset()
        for g in (self.metrics_2d, self.metrics_reprojection, self.metrics_3d):
            g.reset()

    def compute(self) -> Dict[str, Tensor]:
        out = {"heatmap_iou": self.iou_metric.compute()} if self.iou_metric._acc is not None else {}
        for g, dim in ((self.metrics_2d, "2d"), (self.metrics_reprojection, "2d"), (self.metrics_3d, "3d")):
            if g._buf is not None:
                for name, m in zip(g.names, (g.fr005, g.fr01, g.nme)):
                    out[name.format(dim)] = m.compute()
        return out

    @torch.no_grad()
    def __call__(self, outputs: Mapping[str, Tensor], targets: Mapping[str, Tensor]) -> Dict[str, Tensor]:
        res: Dict[str, Tensor] = {}
        bbox = targets[INPUT_BBOX_KEY]
        if OUTPUT_2D_LANDMARKS in outputs.keys() or OUTPUT_LANDMARKS_HEATMAP in outputs.keys():
            res["heatmap_iou"] = self.iou_metric._update_logits(outputs[OUTPUT_LANDMARKS_HEATMAP], targets[TARGET_LANDMARKS_HEATMAP])
            # outputs_2d = _get_keypoints_2d * presence, targets_2d = target * presence * img_size
            if OUTPUT_2D_LANDMARKS in outputs.keys():  # landmarks * img_size
                pred, pred_scale = outputs[OUTPUT_2D_LANDMARKS], self.img_size
            else:  # float(stride) * unravel_index(logits).flip(-1): the argmax of the logits, no sigmoid (flame_lightning_model.py:297)
                pred = float(self.stride) * heatmap_peaks(outputs[OUTPUT_LANDMARKS_HEATMAP], sigmoid=False).flip(-1)
                pred_scale = 1.0
            vals = self.metrics_2d(pred, targets[TARGET_2D_LANDMARKS], bbox, presence=targets[TARGET_2D_LANDMARKS_PRESENCE],
                                   pred_scale=pred_scale, target_scale=self.img_size)
            res.update(zip((n.format("2d") for n in self.metrics_2d.names), vals))
        params = outputs[OUTPUT_3DMM_PARAMS]
        projected = self.head_mesh.reprojected_vertices(params_3dmm=params, to_2d=True)
        vals = self.metrics_reprojection(projected, targets[TARGET_2D_FULL_LANDMARKS], bbox, index=self.face)
        res.update(zip((n.format("2d") for n in self.metrics_reprojection.names), vals))
        pred3d = self.head_mesh.vertices_3d(params_3dmm=params, zero_rotation=True)
        vals = self.metrics_3d(pred3d, targets[TARGET_3D_MODEL_VERTICES], None, index=self.face, cube=True)
        res.update(zip((n.format("3d") for n in self.metrics_3d.names), vals))
        return res
