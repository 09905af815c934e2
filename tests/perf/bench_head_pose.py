#!/usr/bin/env python3
"""Head pose and the scorer's alignment on one MI355X (dad-3dheads_amd/pose.py, csrc/head_pose.hip) beside the host routes they
stand in for, in the same process. Not collected by pytest. Two legs, every figure the median of five repeats with its spread
(min, max); a repeat is the mean of `iters` calls on the host clock, the device synchronised at its end, so a host wait inside
a call is paid where it occurs.

  pose       at 1, 64 and 1024 heads (one 200 x 256 image per head):
               head_pose_s        `pose.head_pose(params)`: rotation matrix + roll / pitch / yaw, one launch
               calculate_rpy_s    `overlay.calculate_rpy(params)`: the rotations copied to the host, scipy once per row
               draw_device_s      `overlay.draw_pose(.., angles="device")`
               draw_host_s        `overlay.draw_pose(.., angles="host")` (calculate_rpy inside)
  evaluate   `evaluation.evaluate_batch` at B = 64 with procrustes="device" and "host"

The numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_head_pose.py [--out profiles/head_pose_bench.json]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import eval_restatement as er  # noqa: E402
from bench_eval import items  # noqa: E402
from dad_3dheads_amd import _lib, evaluation, overlay, pose, synthetic  # noqa: E402
from dad_3dheads_amd.benchmark_export import Landmarks68  # noqa: E402

REPEATS = 5


def wall(fn, iters):
    """{median, min, max} seconds per call over REPEATS repeats of `iters` calls, after one untimed call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / iters)
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times)}


def pose_leg(n):
    h, w = 200, 256
    params = torch.from_numpy(synthetic.synthetic_params(n, seed=n)).cuda()
    torch.manual_seed(n)
    images = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    pred = {"3dmm_params": params}
    iters = 20 if n <= 64 else 3
    res = {"heads": n, "image": [h, w, 3],
           "head_pose_s": wall(lambda: pose.head_pose(params), max(iters, 20)),
           "calculate_rpy_s": wall(lambda: overlay.calculate_rpy(params), iters),
           "draw_device_s": wall(lambda: overlay.draw_pose(pred, images, angles="device"), iters),
           "draw_host_s": wall(lambda: overlay.draw_pose(pred, images, angles="host"), iters)}
    res["rpy_speedup"] = res["calculate_rpy_s"]["median_s"] / res["head_pose_s"]["median_s"]
    res["draw_speedup"] = res["draw_host_s"]["median_s"] / res["draw_device_s"]["median_s"]
    return res


def evaluate_leg(b):
    dev = torch.device("cuda", 0)
    golden, static = er.load_golden(), synthetic.load_static()
    d = items(golden, b, seed=b)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    args = (t(d["gt_vertices"]), t(d["model_view"]), t(d["projection"]), t(d["bbox"].astype(np.float64), torch.float64),
            t(d["height"].astype(np.float32)), t(d["pred_lmk68_2d"]), t(d["pred_vertices"]), t(d["pred_counts"], torch.int32),
            t(d["pred_lmk7"]), t(d["pred_rotation"]))
    kw = dict(landmarks=Landmarks68(static["faces"], device=dev), head_indices=torch.from_numpy(static["head_indices"]).to(dev),
              face_indices=torch.from_numpy(golden["face_indices"].astype(np.int64)).to(dev))
    res = {"B": b,
           "device_s": wall(lambda: evaluation.evaluate_batch(*args, **kw, procrustes="device"), 5),
           "host_s": wall(lambda: evaluation.evaluate_batch(*args, **kw, procrustes="host"), 5)}
    res["speedup"] = res["host_s"]["median_s"] / res["device_s"]["median_s"]
    gt7 = torch.randn(b, 7, 3, dtype=torch.float64, device=dev)
    pred7 = gt7 * 1.1 + 0.01 * torch.randn_like(gt7)
    res["procrustes_batch_s"] = wall(lambda: pose.procrustes_batch(gt7, pred7), 20)
    res["procrustes_host_route_s"] = wall(lambda: [x.to(dev) for x in evaluation.procrustes(gt7.cpu(), pred7.cpu())], 20)
    return res


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "repeats": REPEATS,
           "pose": [pose_leg(n) for n in (1, 64, 1024)], "evaluate": evaluate_leg(64)}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
