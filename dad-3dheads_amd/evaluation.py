"""Scoring side of the DAD-3DHeads accuracy benchmark on the MI355X: `DADEvaluator` of dad_3dheads_benchmark/benchmark.py
(with utils.py) as a batched GPU evaluator.

The four metrics, as the official script computes them (where it differs from its README, this module follows the script):

  pose_error        || I - R_pred . R_gt^T ||_F,  R_gt = (diag(1,-1,-1,1) . MV)[:3,:3]               (benchmark.py:70-82)
  nme_reprojection  100 * mean_i || gt_i - pred_i || / sqrt(bbox[2] * bbox[3]); the GT 68 landmarks are taken on the MODEL-space
                    vertices (`get_68_landmarks`), sent through P . MV, divided by w, y := height - y  (benchmark.py:29-38,84-98)
  z5_accuracy       g = -(GT world head subset), w = predicted head subset (`head_indices`, K = 3669). The script indexes
                    `argsort(cdist(g, g), dim=0)[:, 1:6]`: for the anchors a = head positions 1..5, o_a = all K vertices
                    ordered by distance to g_a (rank 0 included), and vertex i is compared with o_a[i] -- NOT with its own 5
                    nearest neighbours, which is what the README describes (benchmark.py:109-160):
                        Z5 = mean_{i < K, a in 1..5} [(g_z[i] >= g_z[o_a[i]]) == (w_z[i] >= w_z[o_a[i]])]
                    `z5="knn"` opts into the README's definition instead (the 5 nearest OTHER head vertices of each vertex): a
                    deliberate alternative that gives different numbers than the official script.
  chamfer           GT world mesh scaled by 20 / ||lmk68[39] - lmk68[42]|| (landmarks on the world mesh), GT 7 landmarks =
                    lmk68[[36,39,42,45,33,48,54]] of the scaled mesh, Procrustes(gt7, pred7) with reflection="best" (no
                    determinant check: the map may be a reflection), every predicted vertex mapped to b . v . T + c, then the
                    one-sided squared-distance Chamfer mean_q min_p ||q - p||^2 from the 2094 GT face vertices
                    (`flame_indices/face.npy`) to all N aligned predicted vertices (utils.py:119-230). This is kaolin's
                    `chamfer_distance(gt, pred, 1.0, 0.0)` under the ASSUMPTION that its default is `squared=True` (recalled
                    from kaolin 0.12; kaolin is a CUDA extension this project does not depend on, so it is not checked here).

Where the work goes: the 68- and 7-landmark steps and Procrustes (3x3 SVDs) are batched float64 torch; the nearest-neighbour
search (10.5 M pairs per item at N = 5023, the alignment fused into its LDS staging) and the Z5 distance orderings (5 bitonic
sorts of K keys per item) are the HIP kernels of csrc/mesh_eval.hip. Before the fp32 kernels run, the GT face points are centred
on the GT 7-landmark mean and the predicted vertices on their own 7-landmark mean, in float64, so the fp32 distances stay accurate
at world-scale translations (the similarity handed to the kernel absorbs both shifts).

Skipping (benchmark.py:182-195): the script evaluates pose_error, nme, z5, chamfer in that order inside one bare try/except. A
missing ID contributes nothing; a missing key, or an `N_landmarks_3d` too short to index `head_indices`, stops the item at the
failing metric, after the metrics before it were appended; attributes are appended only for items that got all four. Here the
same rule is one explicit decision per item (`metrics_reached`), and every skipped item is counted in `DADEvaluator.warnings`.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import logging
import os
from collections import defaultdict
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib, json_reader
from .benchmark_export import SEVEN_OF_68, Landmarks68
from .projection import project_batch
from .synthetic import load_static

log = logging.getLogger(__name__)

METRICS = (("pose_error", "pose_error"), ("nme", "nme_reprojection"), ("z5", "z5_accuracy"), ("chamfer", "chamfer"))
Z5_ANCHORS = (1, 2, 3, 4, 5)  # `sorted_distances[:, 1:6]` (benchmark.py:133)
INTER_EYE_DIST = 20.0         # scale_gt_to_standard's constant (utils.py:173)
_ROT_180 = (1.0, -1.0, -1.0)  # diag(1,-1,-1,1) of get_gt_rot_mat (benchmark.py:72-76), 3x3 block


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def nearest(query: Tensor, points: Tensor, counts: Optional[Tensor] = None, similarity: Optional[Tensor] = None, k: int = 1,
            self_exclude: bool = False, want_knn: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """Batched one-sided nearest neighbours on the GPU (`dad3d_eval_nearest`).

    query [B,Q,3], points [B,N,3] fp32 CUDA; counts [B] int32 (item b uses its first counts[b] points) or None; similarity
    [B,13] = (s, R 3x3 row-major, t): points are mapped to s * p . R + t first. Returns (min squared distance [B,Q], and with
    `want_knn` the k nearest indices [B,Q,k] int32 and squared distances [B,Q,k], ascending, ties to the lower index)."""
    lib = _lib.load()
    dev = query.device
    assert query.is_cuda and query.dtype == torch.float32 and query.ndim == 3 and query.shape[-1] == 3
    assert points.device == dev and points.dtype == torch.float32 and points.ndim == 3 and points.shape[-1] == 3
    b, q = query.shape[:2]
    n = points.shape[1]
    assert points.shape[0] == b
    query, points = query.contiguous(), points.contiguous()
    if counts is not None:
        counts = counts.to(dev, torch.int32).contiguous()
        assert counts.shape == (b,)
    if similarity is not None:
        similarity = similarity.to(dev, torch.float32).contiguous()
        assert similarity.shape == (b, 13)
    mind = torch.empty((b, q), dtype=torch.float32, device=dev)
    idx = torch.empty((b, q, k), dtype=torch.int32, device=dev) if want_knn else None
    dist = torch.empty((b, q, k), dtype=torch.float32, device=dev) if want_knn else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    flags = _lib.EVAL_SELF_EXCLUDE if self_exclude else 0
    _lib.check(lib.dad3d_eval_nearest(query.data_ptr(), points.data_ptr(), ptr(counts), ptr(similarity), b, q, n, k, flags,
                                      mind.data_ptr(), ptr(idx), ptr(dist), dev.index or 0, _stream(dev)))
    return mind, idx, dist


def z5_ranks(gt_head: Tensor, pred_head: Tensor, anchors: Sequence[int] = Z5_ANCHORS,
             want_order: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """Per-(item, anchor) agreement counts of the script's Z5 (`dad3d_eval_z5_ranks`): gt_head (already negated), pred_head
    [B,K,3] fp32 CUDA -> counts [B,A] int32 (and the orderings o_a [B,A,K] int32 with `want_order`)."""
    lib = _lib.load()
    dev = gt_head.device
    assert gt_head.is_cuda and gt_head.dtype == torch.float32 and gt_head.ndim == 3 and gt_head.shape[-1] == 3
    assert pred_head.shape == gt_head.shape and pred_head.dtype == torch.float32 and pred_head.device == dev
    b, k = gt_head.shape[:2]
    g, w = gt_head.contiguous(), pred_head.contiguous()
    a = (ctypes.c_int32 * len(anchors))(*anchors)
    counts = torch.empty((b, len(anchors)), dtype=torch.int32, device=dev)
    order = torch.empty((b, len(anchors), k), dtype=torch.int32, device=dev) if want_order else None
    _lib.check(lib.dad3d_eval_z5_ranks(g.data_ptr(), w.data_ptr(), b, k, a, len(anchors), counts.data_ptr(),
                                       order.data_ptr() if order is not None else None, dev.index or 0, _stream(dev)))
    return counts, order


def procrustes(x: Tensor, y: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """utils.py:183-272 `procrustes(X, Y)` with scaling and reflection="best" for a batch, float64: X, Y [B,n,3] ->
    (b [B], T [B,3,3], c [B,3]) such that b * Y . T + c best fits X. No determinant check: T may be a reflection."""
    x, y = x.double(), y.double()
    mu_x, mu_y = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
    x0, y0 = x - mu_x, y - mu_y
    norm_x = x0.square().sum((1, 2)).sqrt()
    norm_y = y0.square().sum((1, 2)).sqrt()
    x0 = x0 / norm_x[:, None, None]
    y0 = y0 / norm_y[:, None, None]
    u, s, vt = torch.linalg.svd(x0.transpose(1, 2) @ y0)
    t = vt.transpose(1, 2) @ u.transpose(1, 2)
    b = s.sum(1) * norm_x / norm_y
    c = mu_x[:, 0] - b[:, None] * (mu_y @ t)[:, 0]
    return b, t, c


_procrustes_host = procrustes  # `evaluate_batch` has an argument of the function's name


def evaluate_batch(gt_vertices: Tensor, model_view: Tensor, projection: Tensor, bbox: Tensor, height: Tensor,
                   pred_lmk68_2d: Tensor, pred_vertices: Tensor, pred_counts: Tensor, pred_lmk7: Tensor, pred_rotation: Tensor, *,
                   landmarks: Landmarks68, head_indices: Tensor, face_indices: Tensor, z5: str = "reference",
                   procrustes: str = "host") -> Dict[str, Tensor]:
    """The four benchmark metrics of a batch of items on one device (module docstring).

    GT: gt_vertices [B,5023,3] MODEL-space fp32, model_view / projection [B,4,4], bbox [B,4], height [B].
    Prediction: pred_lmk68_2d [B,68,2], pred_vertices [B,Nmax,3] padded with pred_counts [B] valid rows, pred_lmk7 [B,7,3],
    pred_rotation [B,3,3]. All on the same CUDA device. Returns {"pose_error", "nme", "z5", "chamfer"}: float64 [B] on it.
    An item whose prediction cannot give a metric (short N for Z5, placeholders) gets a meaningless value there: the caller
    decides which values count (`metrics_reached`). `procrustes="device"`: the alignment's 3x3 SVDs run where the landmarks lie
    (`pose.procrustes_batch`), so the batch makes no copy and no wait; "host" (the default) runs them through torch on the CPU.
    The two agree to a few float64 roundings, which can move the last bits of `chamfer` (the similarity is rounded to float32)."""
    if z5 not in ("reference", "knn"):
        raise ValueError(f"z5 must be 'reference' or 'knn', not {z5!r}")
    if procrustes not in ("host", "device"):
        raise ValueError(f"procrustes must be 'host' or 'device', not {procrustes!r}")
    dev = gt_vertices.device
    bsz = gt_vertices.shape[0]
    f32 = lambda t: t.to(dev, torch.float32).contiguous()  # noqa: E731
    gt_vertices, model_view, projection = f32(gt_vertices), f32(model_view), f32(projection)
    height = f32(height)
    head_indices, face_indices = head_indices.to(dev), face_indices.to(dev)

    # GT frame: (MV . [v;1])^T in fp32, HeadAnnotation.from_config (benchmark.py:40-49)
    world = project_batch(gt_vertices, model_view, projection, height, want_world=True)["world"][..., :3]

    # pose_error: float64 like the script (int64 rot_180 @ fp32 MV promotes)
    r_gt = model_view.double()[:, :3, :3] * torch.tensor(_ROT_180, dtype=torch.float64, device=dev)[None, :, None]
    r_dist = pred_rotation.to(dev, torch.float32).double() @ r_gt.transpose(1, 2)
    pose = torch.linalg.matrix_norm(torch.eye(3, dtype=torch.float64, device=dev) - r_dist)

    # nme_reprojection: GT landmarks on the model-space mesh through P . MV, y flipped (the `xy` of project_batch)
    gt2d = project_batch(landmarks(gt_vertices).contiguous(), model_view, projection, height)["xy"]
    bb = bbox.to(dev, torch.float64)
    nme = 100.0 * (gt2d.double() - pred_lmk68_2d.to(dev, torch.float32).double()).norm(dim=-1).mean(1) / (bb[:, 2] * bb[:, 3]).sqrt()

    # z5_accuracy on the head subset
    g = (-world[:, head_indices]).contiguous()
    w = pred_vertices.to(dev, torch.float32)[:, head_indices].contiguous()
    if z5 == "reference":
        counts, _ = z5_ranks(g, w)
        z5v = counts.sum(1).double() / (g.shape[1] * len(Z5_ANCHORS))
    else:
        _, idx, _ = nearest(g, g, k=5, self_exclude=True, want_knn=True)
        idx = idx.long().clamp_min(0)  # K > 5: every query has 5 neighbours
        gz, wz = g[..., 2], w[..., 2]
        agree = (gz[:, :, None] >= torch.gather(gz, 1, idx.flatten(1)).view_as(idx)) == \
                (wz[:, :, None] >= torch.gather(wz, 1, idx.flatten(1)).view_as(idx))
        z5v = agree.double().mean((1, 2))

    # chamfer: scale, 7 landmarks, Procrustes in float64; the alignment is applied inside the nearest-neighbour kernel
    world64 = world.double()
    lmk_w = landmarks(world64)
    scale = INTER_EYE_DIST / (lmk_w[:, 39] - lmk_w[:, 42]).norm(dim=-1)
    gt7 = scale[:, None, None] * lmk_w[:, list(SEVEN_OF_68)]  # = the 7 landmarks of the scaled mesh (linear in the mesh)
    pred7 = pred_lmk7.to(dev, torch.float32).double()
    if procrustes == "device":  # one wave per item: the same bits in any batch, and nothing leaves the device
        from .pose import procrustes_batch
        b, t, c, _ = procrustes_batch(gt7, pred7)
    else:
        b, t, c = (x.to(dev) for x in _procrustes_host(gt7.cpu(), pred7.cpu()))  # 3x3 SVDs on the host: the same bits in any batch
    mu_x, mu_y = gt7.mean(1), pred7.mean(1)
    query = (scale[:, None, None] * world64[:, face_indices] - mu_x[:, None]).float()
    points = (pred_vertices.to(dev, torch.float32).double() - mu_y[:, None]).float()
    # b (p - mu_y) T + t' == b p T + c - mu_x
    shift = c + b[:, None] * (mu_y[:, None] @ t)[:, 0] - mu_x
    sim = torch.cat([b[:, None], t.reshape(bsz, 9), shift], 1).float()
    mind, _, _ = nearest(query, points, pred_counts, sim)
    chamfer = mind.double().mean(1)
    return {"pose_error": pose, "nme": nme, "z5": z5v, "chamfer": chamfer}


def metrics_reached(prediction: Optional[Mapping[str, Any]], n_head_min: int) -> Tuple[int, str]:
    """How many of (pose_error, nme, z5, chamfer) the script appends for an item before its try/except gives up, and why it
    stopped ("" when all four). `n_head_min` = max(head_indices) + 1: the shortest `N_landmarks_3d` that Z5 can index."""
    if prediction is None:
        return 0, "no prediction with this ID"
    checks = (("rotation_matrix", (3, 3)), ("68_landmarks_2d", (68, 2)), ("N_landmarks_3d", None), ("7_landmarks_3d", (7, 3)))
    for i, (key, shape) in enumerate(checks):
        if key not in prediction:
            return i, f"missing {key!r}"
        arr = prediction[key]
        if not isinstance(arr, json_reader.DeviceArray):  # a handle is a regular array of numbers: its .shape and .size, no copy
            try:
                arr = np.asarray(arr, dtype=np.float32)
            except (TypeError, ValueError):
                return i, f"malformed {key!r}"
        if shape is None:  # `torch.Tensor(...).view(-1, 3)[head_indices]` (benchmark.py:152-154)
            if arr.size % 3 or arr.size // 3 < n_head_min:
                return i, f"{key!r} holds {arr.size / 3:g} points; head_indices needs {n_head_min}"
        elif arr.shape != shape:
            return i, f"{key!r} has shape {arr.shape}, not {shape}"
    return 4, ""


def _load_indices(x: Union[str, os.PathLike, np.ndarray, Sequence[int]]) -> np.ndarray:
    if isinstance(x, (str, os.PathLike)):
        return np.load(x).astype(np.int64)
    return np.asarray(x).astype(np.int64)


class DADEvaluator:
    """Drop-in for benchmark.py's `DADEvaluator`: `DADEvaluator(gt_json, submission_json, face_indices=...)()` ->
    (overall_result, attribute_result) as the script returns them, the items batched through `evaluate_batch` on the GPU.

    face_indices: the reference's `model_training/model/static/flame_indices/face.npy` (array or path; reference data, not
    shipped with this package). `z5="knn"` selects the README's nearest-neighbour Z5 (different numbers, module docstring).
    Skipped items are logged and listed in `self.warnings` as (id, reason). `reader="device"` reads both documents through
    `json_reader.load`: the same trees, the arrays of numbers parsed on the GPU and gathered into the batch tensors there.
    `procrustes="device"`: `evaluate_batch`'s alignment on the GPU (no copy, no wait in the batch); the default stays "host"."""

    def __init__(self, ground_truth_path: str, submission_path: str, face_indices, z5: str = "reference", batch_size: int = 64,
                 device: Optional[Union[int, torch.device]] = None, static: Optional[dict] = None, reader: str = "host",
                 procrustes: str = "host"):
        if procrustes not in ("host", "device"):
            raise ValueError(f"procrustes must be 'host' or 'device', not {procrustes!r}")
        self.procrustes = procrustes
        if z5 not in ("reference", "knn"):
            raise ValueError(f"z5 must be 'reference' or 'knn', not {z5!r}")
        if reader not in ("host", "device"):
            raise ValueError(f"reader must be 'host' or 'device', not {reader!r}")
        self.reader = reader
        _lib.require_gpu()
        st = static if static is not None else load_static()
        self.target_file_path = ground_truth_path
        self.prediction_file_path = submission_path
        self.z5 = z5
        self.batch_size = int(batch_size)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.head_indices = st["head_indices"].astype(np.int64)
        self.face_indices = _load_indices(face_indices)
        self.landmarks = Landmarks68(st["faces"], device=self.device)
        self._head = torch.from_numpy(self.head_indices).to(self.device)
        self._face = torch.from_numpy(self.face_indices).to(self.device)
        self.warnings: List[Tuple[str, str]] = []

    def _evaluate(self, items: List[Tuple[Mapping[str, Any], Mapping[str, Any], int]]) -> Dict[str, np.ndarray]:
        """One batch of (annotation, prediction) pairs whose predictions reach at least pose_error; placeholders stand in for
        the fields of the metrics an item does not reach."""
        dev, bsz = self.device, len(items)
        n_min = int(self.head_indices.max()) + 1
        t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
        handle = json_reader.DeviceArray
        shape_of = lambda x: x.shape if isinstance(x, handle) else np.shape(x)  # noqa: E731

        def stack(xs):
            """float32 [B, ...] of one field: handles of one document and one shape are gathered from its values and cast on the
            device (round to nearest even, as np.asarray(list, dtype=np.float32) rounds); lists take the host conversion."""
            first = xs[0]
            if not any(isinstance(x, handle) for x in xs):
                return t(np.stack([np.asarray(x, dtype=np.float32) for x in xs]))
            if all(isinstance(x, handle) and x.document is first.document and x.shape == first.shape for x in xs):
                offsets = torch.tensor([x.offset for x in xs], dtype=torch.int64).to(first.document.values.device)
                index = offsets[:, None] + torch.arange(first.count, device=offsets.device)
                return first.document.values[index].to(torch.float32).view(len(xs), *first.shape).to(dev)
            return torch.stack([x.float32().to(dev) if isinstance(x, handle) else t(np.asarray(x, dtype=np.float32)) for x in xs])

        # predicted vertices, padded to the longest: a handle stays on the device, a list is converted once on the host
        points = [None if reach <= 2 else p["N_landmarks_3d"] if isinstance(p["N_landmarks_3d"], handle)
                  else np.asarray(p["N_landmarks_3d"], dtype=np.float32).reshape(-1, 3) for _, p, reach in items]
        n_pts = [0 if v is None else v.count // 3 if isinstance(v, handle) else len(v) for v in points]
        n_max = max(1, n_min, max(n_pts))
        if not any(isinstance(v, handle) for v in points):
            host = np.zeros((bsz, n_max, 3), np.float32)
            for i, v in enumerate(points):
                if v is not None:
                    host[i, :len(v)] = v
            pv = t(host)
        else:
            pv = torch.zeros((bsz, n_max, 3), dtype=torch.float32, device=dev)
            if all(isinstance(v, handle) for v in points) and len(set(n_pts)) == 1:
                pv[:, :n_pts[0]] = stack(points).view(bsz, -1, 3)
            else:
                for i, v in enumerate(points):
                    if v is not None:
                        pv[i, :n_pts[i]] = v.float32().to(dev).view(-1, 3) if isinstance(v, handle) else t(v)
        # placeholders for the fields of metrics an item does not reach; non-degenerate, so Procrustes' SVD stays finite
        field = lambda p, key, shape: (p[key] if key in p and shape_of(p[key]) == shape else np.eye(*shape, dtype=np.float32))  # noqa: E731
        out = evaluate_batch(
            stack([a["vertices"] for a, _, _ in items]),
            stack([a["model_view_matrix"] for a, _, _ in items]),
            stack([a["projection_matrix"] for a, _, _ in items]),
            t(np.asarray([a["bbox"] for a, _, _ in items], dtype=np.float64), torch.float64),
            t(np.asarray([a["image_height"] for a, _, _ in items], dtype=np.float32)),
            stack([field(p, "68_landmarks_2d", (68, 2)) for _, p, _ in items]),
            pv, t(np.asarray(n_pts, dtype=np.int32), torch.int32),
            stack([field(p, "7_landmarks_3d", (7, 3)) for _, p, _ in items]),
            stack([field(p, "rotation_matrix", (3, 3)) for _, p, _ in items]),
            landmarks=self.landmarks, head_indices=self._head, face_indices=self._face, z5=self.z5, procrustes=self.procrustes)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def __call__(self) -> Tuple[Dict[str, float], Dict[str, Dict[str, Dict[Any, float]]]]:
        if self.reader == "device":  # the arrays of numbers stay on the device as handles (json_reader.py)
            submission = json_reader.load(self.prediction_file_path, self.device).root
            ground_truth = json_reader.load(self.target_file_path, self.device).root
        else:
            with open(self.prediction_file_path) as f:
                submission = json.load(f)
            with open(self.target_file_path) as f:
                ground_truth = json.load(f)
        n_min = int(self.head_indices.max()) + 1
        self.warnings = []
        lists = {name: [] for name, _ in METRICS}
        attrs = {name: defaultdict(lambda: defaultdict(list)) for name, _ in METRICS}
        work: List[Tuple[Mapping[str, Any], Mapping[str, Any], int]] = []
        for anno in ground_truth:
            pred = submission.get(anno["id"])
            reach, why = metrics_reached(pred, n_min)
            if reach < len(METRICS):
                self.warnings.append((str(anno["id"]), why))
                log.warning("item %s: %s (%d of %d metrics counted)", anno["id"], why, reach, len(METRICS))
            if reach:
                work.append((anno, pred, reach))
        for start in range(0, len(work), self.batch_size):
            chunk = work[start:start + self.batch_size]
            vals = self._evaluate(chunk)
            for i, (anno, _, reach) in enumerate(chunk):
                sample = {name: float(vals[name][i]) for name, _ in METRICS[:reach]}
                for name, v in sample.items():
                    lists[name].append(v)
                if reach == len(METRICS) and anno.get("attributes") is not None:
                    for attr_name, attr_value in anno["attributes"].items():
                        for name, v in sample.items():
                            attrs[name][attr_name][attr_value].append(v)
        mean = lambda v: float(np.mean(v)) if len(v) else float("nan")  # noqa: E731
        overall = {out: mean(lists[name]) for name, out in METRICS}
        attribute = {out: {a: {val: mean(vs) for val, vs in per.items()} for a, per in attrs[name].items()} for name, out in METRICS}
        return overall, attribute


def summary_text(overall: Mapping[str, float], attribute: Mapping[str, Mapping[str, Mapping[Any, float]]]) -> str:
    """Plain-text view of the two result dicts."""
    lines = [f"{name:<20} {value:>12.6f}" for name, value in overall.items()]
    for metric, per_attr in attribute.items():
        for attr, values in per_attr.items():
            for val, v in sorted(values.items(), key=lambda kv: str(kv[0])):
                lines.append(f"{metric:<20} {attr}={val}: {v:.6f}")
    return "\n".join(lines)


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description="Score a DAD-3DHeads submission JSON against a ground-truth JSON on the GPU.")
    ap.add_argument("--submission", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--face-indices", required=True, help="flame_indices/face.npy of the reference model data")
    ap.add_argument("--z5", choices=("reference", "knn"), default="reference")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--reader", choices=("host", "device"), default="host", help="device: parse the arrays of numbers of both files on the GPU")
    ap.add_argument("--procrustes", choices=("host", "device"), default="host", help="device: the alignment's 3x3 SVDs on the GPU")
    args = ap.parse_args(argv)
    ev = DADEvaluator(args.gt, args.submission, face_indices=args.face_indices, z5=args.z5, batch_size=args.batch_size, reader=args.reader,
                      procrustes=args.procrustes)
    overall, attribute = ev()
    print(summary_text(overall, attribute))
    if ev.warnings:
        print(f"{len(ev.warnings)} item(s) skipped in part or whole")


if __name__ == "__main__":
    main()
