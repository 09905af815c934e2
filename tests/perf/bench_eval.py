#!/usr/bin/env python3
"""Throughput of the benchmark scorer (dad-3dheads_amd/evaluation.py) on one MI355X, beside the float64 CPU restatement of
tests/eval_restatement.py on the same items. Not collected by pytest.

Items: the three complete items of tests/golden/eval_golden.npz, repeated with fresh prediction noise to B. Reported per B:
  json_parse_s         json.loads of the GT + submission documents (what DADEvaluator reads), measured on min(B, 64) items and
                       scaled to B (1024 items are ~1 GB of JSON text)
  host_s               evaluate_batch's inputs from the parsed lists (np.asarray) + the host Procrustes, scaled the same way
  kernel_s             the two kernels alone (nearest neighbours with the fused alignment, Z5 anchor ranks), CUDA events
  evaluate_batch_s     evaluate_batch end to end on device tensors (synchronised)
  items_per_s_*        B / the matching time; the CPU restatement on a subset of items

    python tests/perf/bench_eval.py [B ...] [--out profiles/eval_bench.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import eval_restatement as er  # noqa: E402
from dad_3dheads_amd import _lib, evaluation, synthetic  # noqa: E402
from dad_3dheads_amd.benchmark_export import Landmarks68  # noqa: E402
from event_timer import event_time  # noqa: E402


def items(golden, b, seed):
    rng = np.random.default_rng(seed)
    src = np.arange(b) % 3
    d = {k: golden[k][src].copy() for k in ("gt_vertices", "model_view", "projection", "bbox", "height", "pred_vertices",
                                            "pred_counts", "pred_lmk68_2d", "pred_lmk7", "pred_rotation")}
    d["pred_vertices"] += rng.normal(0, 5e-4, d["pred_vertices"].shape).astype(np.float32)
    d["pred_vertices"][np.arange(d["pred_vertices"].shape[1])[None, :] >= d["pred_counts"][:, None]] = 0
    d["pred_lmk68_2d"] += rng.normal(0, 1.0, d["pred_lmk68_2d"].shape).astype(np.float32)
    return d


def documents(golden, d):
    attrs = json.loads(str(golden["attributes"]))
    g = dict(golden, **d, attributes=np.array(json.dumps([attrs[i % 3] for i in range(len(d["height"]))])),
             has_7=np.ones(len(d["height"]), np.int8), has_pred=np.ones(len(d["height"]), np.int8))
    gt, sub = er.golden_json(g)
    return json.dumps(gt), json.dumps(sub)


def run(golden, static, b, iters):
    dev = torch.device("cuda", 0)
    d = items(golden, b, seed=b)
    m = min(b, 64)
    gt_text, sub_text = documents(golden, {k: v[:m] for k, v in d.items()})
    t0 = time.perf_counter()
    gt, sub = json.loads(gt_text), json.loads(sub_text)
    t_json = (time.perf_counter() - t0) * b / m

    t0 = time.perf_counter()
    arrays = {
        "gt_vertices": np.stack([np.asarray(a["vertices"], np.float32) for a in gt]),
        "model_view": np.stack([np.asarray(a["model_view_matrix"], np.float32) for a in gt]),
        "projection": np.stack([np.asarray(a["projection_matrix"], np.float32) for a in gt]),
        "pred_vertices": np.stack([np.pad(np.asarray(sub[a["id"]]["N_landmarks_3d"], np.float32),
                                          ((0, d["pred_vertices"].shape[1] - len(sub[a["id"]]["N_landmarks_3d"])), (0, 0))) for a in gt]),
        "pred_lmk68_2d": np.stack([np.asarray(sub[a["id"]]["68_landmarks_2d"], np.float32) for a in gt]),
        "pred_lmk7": np.stack([np.asarray(sub[a["id"]]["7_landmarks_3d"], np.float32) for a in gt]),
        "pred_rotation": np.stack([np.asarray(sub[a["id"]]["rotation_matrix"], np.float32) for a in gt]),
    }
    evaluation.procrustes(torch.from_numpy(arrays["pred_lmk7"]).double(), torch.from_numpy(arrays["pred_lmk7"]).double() * 1.1)
    t_host = (time.perf_counter() - t0) * b / m

    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    assert np.array_equal(arrays["gt_vertices"], d["gt_vertices"][:m]) and np.array_equal(arrays["pred_vertices"], d["pred_vertices"][:m])
    args = (t(d["gt_vertices"]), t(d["model_view"]), t(d["projection"]), t(d["bbox"].astype(np.float64), torch.float64),
            t(d["height"].astype(np.float32)), t(d["pred_lmk68_2d"]), t(d["pred_vertices"]), t(d["pred_counts"], torch.int32),
            t(d["pred_lmk7"]), t(d["pred_rotation"]))
    kw = dict(landmarks=Landmarks68(static["faces"], device=dev), head_indices=torch.from_numpy(static["head_indices"]).to(dev),
              face_indices=torch.from_numpy(golden["face_indices"].astype(np.int64)).to(dev))
    t_eval = event_time(lambda: evaluation.evaluate_batch(*args, **kw), iters, 1)

    # the kernels alone, on inputs of the evaluated shapes
    face = torch.randn(b, 2094, 3, device=dev)
    pts = args[6]
    sim = torch.zeros(b, 13, device=dev)
    sim[:, 0] = 1.0
    sim[:, 1:10] = torch.eye(3, device=dev).reshape(9)
    head = kw["head_indices"]
    g, w = pts[:, head].contiguous(), pts[:, head].contiguous()
    t_nn = event_time(lambda: evaluation.nearest(face, pts, args[7], sim), iters, 1)
    t_z5 = event_time(lambda: evaluation.z5_ranks(g, w), iters, 1)
    return {"B": b, "json_parse_s": t_json, "host_s": t_host, "kernel_nearest_s": t_nn, "kernel_z5_s": t_z5,
            "evaluate_batch_s": t_eval, "items_per_s_evaluate_batch": b / t_eval, "items_per_s_kernels": b / (t_nn + t_z5),
            "items_per_s_with_json": b / (t_json + t_host + t_eval), "max_counts": int(d["pred_counts"].max())}


def cpu_restatement(golden, n):
    r = er.restatement_from_package(golden["face_indices"])
    d = items(golden, n, seed=1)
    t0 = time.perf_counter()
    for i in range(n):
        world = r.world(d["gt_vertices"][i], d["model_view"][i])
        pv = d["pred_vertices"][i, :d["pred_counts"][i]]
        r.pose_error(d["model_view"][i], d["pred_rotation"][i])
        r.nme(d["gt_vertices"][i], d["model_view"][i], d["projection"][i], d["bbox"][i], d["height"][i], d["pred_lmk68_2d"][i])
        r.z5(world, pv)
        r.chamfer(world, pv, d["pred_lmk7"][i])
    dt = time.perf_counter() - t0
    return {"items": n, "seconds": dt, "items_per_s": n / dt}


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    sizes = [int(x) for x in argv] or [64, 1024]
    _lib.require_gpu()
    torch.cuda.set_device(0)
    golden = er.load_golden()
    static = synthetic.load_static()
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
           "gpu": [run(golden, static, b, iters=5 if b > 256 else 20) for b in sizes],
           "cpu_float64_restatement": cpu_restatement(golden, 4)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
