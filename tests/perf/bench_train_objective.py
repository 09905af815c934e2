#!/usr/bin/env python3
"""Throughput of the training-objective kernels (csrc/train_objective.hip) on one MI355X, each beside its baseline from the
same process. Not collected by pytest.

Per B in (64, 256), C = 68 heatmaps of 64 x 64 (img_size 256, stride 4), CUDA events after warm-up:
  iou_fused_s           IoULoss forward + backward (uint8 target, what the dataset stores), through autograd, eager
  iou_fused_graph_s     the same step replayed from a captured graph (no host work per launch)
  iou_fwd_s / iou_bwd_s the two C entries alone (terms + finish; gradient)
  iou_torch_s           the reference's torch statement (keypoint_losses.py:11-30) forward + backward on the fp32 target
  iou_*_gbps            algorithmic bytes / time: forward = logits + uint8 target, backward = those again + the fp32 gradient
  encode_s              HeatmapCoder.encode (uint8 form) of one batch on the GPU
  encode_cpu_loop_s     the reference coder's per-sample loop, restated in NumPy (tests/train_objective_restatement.encode),
                        plus `np.uint8(255 * h)`; `h2d_copy_s` = copying its 17.8 MB (B = 64) of bytes to the device
  objective_s           LossModule with the four HIP criteria of train_loss.yaml, forward + backward
  objective_baseline_s  the same module with the torch statements for the heatmap and landmark terms (HIP mesh losses)

    python tests/perf/bench_train_objective.py [--out profiles/train_objective_bench.json] [--quick]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import train_objective_restatement as R  # noqa: E402
from dad_3dheads_amd import _lib, synthetic  # noqa: E402
from dad_3dheads_amd.coder import HeatmapCoder  # noqa: E402
from dad_3dheads_amd.flame import FLAME_CONSTS  # noqa: E402
from dad_3dheads_amd.loss_module import LossModule  # noqa: E402
from dad_3dheads_amd.losses import IoULoss  # noqa: E402
from event_timer import event_time  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


class TorchIoU(torch.nn.Module):
    """keypoint_losses.py:5-30, the reference's statement."""

    def forward(self, y_pred, y_true):
        def op_sum(x):
            return x.view(x.shape[0], x.shape[1], -1).sum(2)

        y = torch.sigmoid(y_pred)
        t = y_true.div(255.0) if y_true.dtype == torch.uint8 else y_true  # get_input's uint8_to_float32
        iou = (op_sum(t * y) + 1e-6) / (op_sum(t ** 2) + op_sum(y ** 2) - op_sum(t * y) + 1e-6)
        return 1 - torch.mean(iou)


class TorchLandmarks(torch.nn.Module):
    """landmarks_loss_w_visibility.py:17-26 with SmoothL1."""

    def forward(self, predicted, target):
        return torch.nn.functional.smooth_l1_loss(predicted[0] * predicted[1][..., None], target[0] * target[1][..., None])


def iou_leg(b, iters):
    c, s = 68, 64
    n = b * c * s * s
    logits, t8 = R.iou_inputs(b, b, c, s, s)
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    t = torch.from_numpy(t8).cuda()
    tf = t.float().div(255.0)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    sums = torch.empty((b * c, 3), dtype=torch.float64, device="cuda")
    out = torch.empty(2, device="cuda")
    one = torch.ones(1, device="cuda")
    grad = torch.empty_like(x)

    crit = IoULoss()

    def fused():
        x.grad = None
        crit(x, t).backward()

    def fwd():
        lib.dad3d_heatmap_iou(x.data_ptr(), t.data_ptr(), 1, b, c, s * s, 1, sums.data_ptr(), None, out.data_ptr(), None, 0, stream)

    def bwd():
        lib.dad3d_heatmap_iou_grad(x.data_ptr(), t.data_ptr(), 1, b, c, s * s, sums.data_ptr(), one.data_ptr(), grad.data_ptr(), 0, stream)

    ref = TorchIoU()

    def torch_stmt():
        x.grad = None
        ref(x, tf).backward()

    res = {"batch": b, "channels": c, "hw": s * s}
    res["iou_fused_s"] = event_time(fused, iters, 3)
    # the same autograd step replayed from a graph: the device time without the host's per-launch work
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fused()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        crit(x, t).backward()
    res["iou_fused_graph_s"] = event_time(graph.replay, iters, 3)
    x.grad = None
    res["iou_fwd_s"] = event_time(fwd, iters, 3)
    res["iou_bwd_s"] = event_time(bwd, iters, 3)
    res["iou_torch_s"] = event_time(torch_stmt, iters, 3)
    fwd_bytes, bwd_bytes = 5 * n, 9 * n
    res.update({"fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
                "iou_fwd_gbps": fwd_bytes / res["iou_fwd_s"] / 1e9, "iou_bwd_gbps": bwd_bytes / res["iou_bwd_s"] / 1e9,
                "iou_pair_share_of_hbm": (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S / (res["iou_fwd_s"] + res["iou_bwd_s"]),
                "iou_fused_vs_torch": res["iou_torch_s"] / res["iou_fused_s"],
                "iou_kernels_vs_torch": res["iou_torch_s"] / (res["iou_fwd_s"] + res["iou_bwd_s"])})
    return res


def encode_leg(b, iters, cpu_reps):
    rng = np.random.default_rng(b)
    kp = rng.uniform(0, 256, (b, 68, 2)).astype(np.float32)
    pr = rng.random((b, 68)) < 0.9
    coder = HeatmapCoder({"img_size": 256, "stride": 4, "radius": 5}, 68)
    kd, pd = torch.from_numpy(kp).cuda(), torch.from_numpy(pr).cuda()
    out = torch.empty((b, 68, 64, 64), dtype=torch.uint8, device="cuda")
    res = {"batch": b, "encode_s": event_time(lambda: coder.encode(kd, pd, form="uint8", out=out), iters, 3)}
    res["encode_bytes"] = out.numel()
    res["encode_gbps"] = out.numel() / res["encode_s"] / 1e9
    t0 = time.perf_counter()
    for _ in range(cpu_reps):
        u8 = np.uint8(255.0 * R.encode(kp, pr, 64, 4, 5, "raw"))
    res["encode_cpu_loop_s"] = (time.perf_counter() - t0) / cpu_reps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(cpu_reps):
        torch.from_numpy(u8).cuda()
    torch.cuda.synchronize()
    res["h2d_copy_s"] = (time.perf_counter() - t0) / cpu_reps
    res["encode_vs_cpu_loop"] = res["encode_cpu_loop_s"] / res["encode_s"]
    return res


def objective_leg(b, iters):
    model = synthetic.synthetic_flame_model(0, synthetic.load_static())
    static = synthetic.load_static()
    d = tempfile.mkdtemp()
    regions = {"face": np.arange(0, 5023, 3), "face_w_ears": np.arange(0, 5023, 2), "head": np.arange(5023)}
    for k, v in regions.items():
        np.save(os.path.join(d, k + ".npy"), v)
    folder = {"folder": d, "files": {k: k + ".npy" for k in regions}}
    crit = [
        {"name": "heatmap_loss", "target_key": "TARGET_LANDMARKS_HEATMAP", "output_key": "OUTPUT_LANDMARKS_HEATMAP", "weight": 1.,
         "loss": {"_target_": "model_training.losses.IoULoss"}},
        {"name": "vertices3d_loss", "target_key": "TARGET_3D_MODEL_VERTICES", "output_key": "OUTPUT_3DMM_PARAMS", "weight": 50.,
         "loss": {"_target_": "model_training.losses.Vertices3DLoss", "criterion": "l2", "batch_size": b, "consts": FLAME_CONSTS,
                  "weights_and_indices": {"flame_indices": folder, "weights": {"head": .5, "face_w_ears": .75, "face": 1.}}}},
        {"name": "reprojection_loss", "target_key": "TARGET_2D_FULL_LANDMARKS", "output_key": "OUTPUT_3DMM_PARAMS", "weight": 0.05,
         "loss": {"_target_": "model_training.losses.ReprojectionLoss", "criterion": "smooth_l1", "batch_size": b, "consts": FLAME_CONSTS,
                  "img_size": 256, "weights_and_indices": {"flame_indices": folder, "weights": {"face": .5, "face_w_ears": .5}}}},
        {"name": "landmarks_loss", "target_key": ["TARGET_2D_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE"],
         "output_key": ["OUTPUT_2D_LANDMARKS", "TARGET_2D_LANDMARKS_PRESENCE"], "weight": 100.,
         "loss": {"_target_": "model_training.losses.LandmarksLossWVisibility", "criterion": "smooth_l1"}}]
    hip = LossModule.from_config({"criterions": crit}, head_mesh_kwargs={"flame_model": model, "static": static, "device": 0})
    base = LossModule(hip.names, hip.output_keys, hip.target_keys,
                      [TorchIoU(), hip.criterions[1], hip.criterions[2], TorchLandmarks()], hip.weights, hip.schedule)
    rng = np.random.default_rng(b)
    logits, t8 = R.iou_inputs(b + 1, b, 68, 64, 64)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=b)).cuda()
    dec = torch.from_numpy(synthetic.synthetic_params(b, seed=b + 7)).cuda()
    from dad_3dheads_amd.head_mesh import HeadMesh

    hm = HeadMesh(flame_model=model, static=static, device=0)
    with torch.no_grad():
        tgt3d = hm.vertices_3d(dec.clone(), zero_rotation=True)
        tgt2d = hm.reprojected_vertices(dec.clone(), to_2d=True)
    targets = {"TARGET_LANDMARKS_HEATMAP": torch.from_numpy(t8).cuda(), "TARGET_3D_MODEL_VERTICES": tgt3d,
               "TARGET_2D_FULL_LANDMARKS": tgt2d, "TARGET_2D_LANDMARKS": torch.from_numpy(rng.uniform(0, 1, (b, 68, 2)).astype(np.float32)).cuda(),
               "TARGET_2D_LANDMARKS_PRESENCE": torch.from_numpy((rng.random((b, 68)) < 0.9).astype(np.float32)).cuda()}
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    p = params.clone().requires_grad_(True)
    lmk = torch.from_numpy(rng.uniform(0, 1, (b, 68, 2)).astype(np.float32)).cuda().requires_grad_(True)

    def run(module):
        def f():
            x.grad = p.grad = lmk.grad = None
            total, _ = module({"OUTPUT_LANDMARKS_HEATMAP": x, "OUTPUT_3DMM_PARAMS": p * 1.0, "OUTPUT_2D_LANDMARKS": lmk}, targets, 0)
            total.backward()
        return f

    res = {"batch": b, "objective_s": event_time(run(hip), iters, 3), "objective_baseline_s": event_time(run(base), iters, 3)}
    res["objective_vs_baseline"] = res["objective_baseline_s"] / res["objective_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_objective_bench.json"))
    ap.add_argument("--quick", action="store_true", help="few iterations (for a profiler run)")
    args = ap.parse_args()
    iters = 5 if args.quick else 50
    result = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "iou": [], "encode": [], "objective": []}
    for b in (64, 256):
        result["iou"].append(iou_leg(b, iters))
        result["encode"].append(encode_leg(b, iters, 1 if args.quick else 3))
        result["objective"].append(objective_leg(b, max(5, iters // 5)))
        print(json.dumps({"batch": b, "iou": result["iou"][-1], "encode": result["encode"][-1], "objective": result["objective"][-1]}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
