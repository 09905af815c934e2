#!/usr/bin/env python3
"""Throughput of the device-built training batch (dataset.FlameBatchBuilder) on one MI355X. Not collected by pytest.

Per B in (64, 256): crop sides drawn log-uniform in [64, 640] px per axis (train_batch_restatement.crop_sides, seed 0),
68-landmark mode, longest_max_size + imagenet, S = 256, stride 4. CUDA events after warm-up, per batch:
  h2d_s        the pinned raw batch to the device (crops + vertices + matrices + descriptors), one stream
  image_s      dad3d_preprocess_images alone
  keypoints_s  dad3d_gt_keypoints alone
  heatmap_s    HeatmapCoder.encode (uint8) alone
  builder_s    the whole FlameBatchBuilder call from pinned memory (H2D + the three launches + the small descriptor add)
  *_bytes      algorithmic bytes; *_tbps / h2d_gbps = bytes / time (HBM peak 8 TB/s; PCIe Gen5 x16 ~64 GB/s per direction)
  cpu_restatement_s   tests/train_batch_restatement.chain (NumPy) over the batch's keypoints, plus oracle-free image work is
                      NOT included: a stand-in for the loader's geometry only. albumentations' own per-keypoint cost cannot be
                      measured here (the package is not installed), so no number is given for it.

    python tests/perf/bench_train_batch.py [--out profiles/train_batch_bench.json] [--quick]
"""
import argparse
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
import train_batch_restatement as rs  # noqa: E402
from dad_3dheads_amd import synthetic  # noqa: E402
from dad_3dheads_amd.dataset import RESIZE_MODES, FlameBatchBuilder, RawBatchCollate  # noqa: E402
from event_timer import event_time  # noqa: E402

CONFIG = {"img_size": 256, "stride": 4, "num_classes": 68, "keypoints": {"2d_subset_name": "multipie_keypoints"},
          "transform": {"normalize": "imagenet", "resize_mode": "longest_max_size"}}


def raw_items(b, st, seed=0):
    rng = np.random.default_rng(seed)
    sides = rs.crop_sides(rng, b)
    items = []
    for i, (h, w) in enumerate(sides):
        ih, iw = int(h) + 40, int(w) + 40
        mv, pm = rs.camera(seed * 1000 + i, ih, iw, 0.7 * min(h, w), (iw / 2, ih / 2))
        img = rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8)
        items.append({"image": img, "bbox": np.array([20, 20, w, h], np.int32), "image_shape": np.array([ih, iw, 3]),
                      "vertices": rs.mesh(i, st["template_geo"]), "model_view": mv, "projection": pm, "SAMPLE_INDEX_KEY": i,
                      "IMAGE_FILENAME_KEY": f"{i}.png"})
    return items, sides


def bench(b, iters, st):
    dev = torch.device("cuda", 0)
    builder = FlameBatchBuilder(CONFIG, 0)
    items, sides = raw_items(b, st)
    raw = RawBatchCollate(256)(items)
    raw = {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in raw.items()}
    up = {k: v.to(dev) for k, v in raw.items() if torch.is_tensor(v)}
    lib, s = builder._lib, torch.cuda.current_stream(dev).cuda_stream
    descs = up["crop_descs"].clone()
    descs[:, 0] += up["crops"].data_ptr()
    n, k = up["vertices"].shape[1], 68
    images = torch.empty((b, 3, 256, 256), device=dev)
    full, px, norm = (torch.empty((b, m, 2), device=dev) for m in (n, k, k))
    pres = torch.empty((b, k), dtype=torch.uint8, device=dev)
    h2d_bytes = sum(v.numel() * v.element_size() for v in raw.values() if torch.is_tensor(v))

    def h2d():
        for key, v in raw.items():
            if torch.is_tensor(v):
                up[key].copy_(v, non_blocking=True)

    def image():
        lib.dad3d_preprocess_images(descs.data_ptr(), b, 256, builder._mean, builder._std, images.data_ptr(), 0, s)

    def keypoints():
        lib.dad3d_gt_keypoints(up["vertices"].data_ptr(), up["model_view"].data_ptr(), up["projection"].data_ptr(),
                               up["frames"].data_ptr(), b, n, None, builder.corners.data_ptr(), builder.weights.data_ptr(), k, 256,
                               RESIZE_MODES["longest_max_size"], full.data_ptr(), px.data_ptr(), norm.data_ptr(), pres.data_ptr(), 0, s)

    def heatmap():
        builder.coder.encode(px, pres, form="uint8")

    def whole():
        builder(raw)

    keypoints()
    out = {"batch": b, "crop_sides": "log-uniform [64, 640] px per axis, seed 0",
           "crop_side_median": float(np.median(sides)), "crop_bytes": int(raw["crops"].numel())}
    out["h2d_s"] = event_time(h2d, iters, 3)
    out["image_s"] = event_time(image, iters, 3)
    out["keypoints_s"] = event_time(keypoints, iters, 3)
    out["heatmap_s"] = event_time(heatmap, iters, 3)
    out["builder_s"] = event_time(whole, iters, 3)
    taps = int(sum(min(int(h), 256) * min(int(w), 256) for h, w in sides)) * 3  # bytes the resize can touch (<= crop)
    out["h2d_bytes"], out["h2d_gbps"] = h2d_bytes, h2d_bytes / out["h2d_s"] / 1e9
    out["image_bytes"] = b * 3 * 256 * 256 * 4 + taps
    out["keypoints_bytes"] = b * (n * 12 + n * 8 + k * (36 + 8 + 8 + 1) + 128 + 32)
    out["heatmap_bytes"] = b * k * 64 * 64 + b * k * 9
    for key in ("image", "keypoints", "heatmap"):
        out[key + "_tbps"] = out[key + "_bytes"] / out[key + "_s"] / 1e12
    corners, weights = rs.lmk68_tables(st)
    t0 = time.perf_counter()
    for it in items:
        frame = (it["image_shape"][0], *it["bbox"])
        rs.chain(it["vertices"], it["model_view"], it["projection"], frame, 256, "longest_max_size", corners=corners, weights=weights)
    out["cpu_restatement_s"] = time.perf_counter() - t0
    out["cpu_restatement_note"] = "NumPy restatement of the keypoint chain for the batch, one process: a stand-in for the loader"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batch_bench.json"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    st = synthetic.load_static()
    res = {"device": torch.cuda.get_device_name(0), "iters": 5 if args.quick else 50,
           "albumentations_note": "albumentations is not installed: its per-keypoint cost is not measured and not estimated",
           "runs": [bench(b, 5 if args.quick else 50, st) for b in (64, 256)]}
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
