#!/usr/bin/env python3
"""The file form of the training loader against the raw form, on one MI355X and its host. Not collected by pytest.

Per B in (64, 256): PNG photos (crops of the demo photograph, mirrored to size) whose bbox sides are the ones bench_train_batch.py
draws (log-uniform in [64, 640] px per axis, seed 0, 20 px of margin), one 5 023-vertex annotation each as `json.dumps` writes it,
68-landmark mode, longest_max_size + imagenet, S = 256. Everything is timed in this one process:
  getitem_raw_s / getitem_files_s   per-item CPU time of `FlameDataset.__getitem__` in both forms (files in the page cache)
  collate_raw_s / collate_files_s   per-batch CPU time of the two collates
  bus_bytes_raw / bus_bytes_files   what a batch uploads in each form
  raw_builder_s                     the parent's raw form, FlameBatchBuilder from pinned memory (no host sync)
  files_builder_s                   the file form, FlameBatchBuilder from pinned memory: wall clock, its one sync included
  files_h2d_s, files_png_s, files_annotation_s, files_rest_s
                                    the file form's parts between events: the uploads, `dad3d_png_decode`, `dad3d_annotation_parse`,
                                    and the three kernels both forms share (with the crop descriptors built in place)
  annotation_bound_s                the annotation kernel's streaming bound: text bytes over HBM's achievable rate (6.3 TB/s;
                                    the spec is 8 TB/s) -- the kernel reads each byte once and writes 60 KB per document
None of this is a pass or fail bar.

    python tests/perf/bench_train_files.py [--out profiles/train_files_bench.json] [--quick]
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
import train_batch_restatement as rs  # noqa: E402
from dad_3dheads_amd import synthetic  # noqa: E402
from dad_3dheads_amd.dataset import FlameBatchBuilder, FlameDataset  # noqa: E402
from event_timer import event_time  # noqa: E402

CONFIG = {"img_size": 256, "stride": 4, "num_classes": 68, "keypoints": {"2d_subset_name": "multipie_keypoints"},
          "transform": {"normalize": "imagenet", "resize_mode": "longest_max_size"}}
HBM_ACHIEVABLE = 6.3e12


def write_files(root, b, st, seed=0):
    from PIL import Image

    with np.load(os.path.join(ROOT, "tests", "golden", "demo_image.npz")) as z:
        photo = z["resized"]
    big = np.pad(photo, ((0, max(0, 800 - photo.shape[0])), (0, max(0, 800 - photo.shape[1])), (0, 0)), mode="symmetric")
    rng = np.random.default_rng(seed)
    anno = []
    for i, (h, w) in enumerate(rs.crop_sides(rng, b)):
        ih, iw = int(h) + 40, int(w) + 40
        oy, ox = i % (big.shape[0] - ih + 1), (7 * i) % (big.shape[1] - iw + 1)
        Image.fromarray(np.ascontiguousarray(big[oy:oy + ih, ox:ox + iw])).save(os.path.join(root, f"{i}.png"))
        mv, pm = rs.camera(seed * 1000 + i, ih, iw, 0.7 * min(h, w), (iw / 2, ih / 2))
        doc = {"vertices": rs.mesh(i, st["template_geo"]).astype(np.float64).tolist(), "model_view_matrix": mv.astype(np.float64).tolist(),
               "projection_matrix": pm.astype(np.float64).tolist()}
        with open(os.path.join(root, f"{i}.json"), "w") as f:
            json.dump(doc, f)
        # the jitter grows a side by 10 .. 30 %: a bbox of 1 / 1.2 of the drawn side keeps the crops at bench_train_batch's sizes
        bw, bh = int(w / 1.2), int(h / 1.2)
        anno.append({"img_path": f"{i}.png", "bbox": [20 + (int(w) - bw) // 2, 20 + (int(h) - bh) // 2, bw, bh], "annotation_path": f"{i}.json"})
    return anno


def per_item(ds, repeats):
    best = float("inf")
    for _ in range(repeats):
        np.random.seed(0)
        t0 = time.perf_counter()
        items = [ds[i] for i in range(len(ds))]
        best = min(best, (time.perf_counter() - t0) / len(ds))
    return best, items


def host_time(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def tensor_bytes(batch):
    return int(sum(v.numel() * v.element_size() for v in batch.values() if torch.is_tensor(v)))


def bench(b, iters, st, root):
    dev = torch.device("cuda", 0)
    cfg = dict(CONFIG, dataset_root=root)
    anno = write_files(root, b, st)
    raw_ds, file_ds = FlameDataset(anno, cfg), FlameDataset(anno, cfg, item_form="files")
    out = {"batch": b, "images": "demo photograph, mirrored; bbox sides log-uniform [64, 640] px / 1.2, seed 0"}
    out["getitem_raw_s"], raw_items = per_item(raw_ds, 2)
    out["getitem_files_s"], file_items = per_item(file_ds, 2)
    pin = lambda batch: {k: (v.pin_memory() if torch.is_tensor(v) else v) for k, v in batch.items()}  # noqa: E731
    t0 = time.perf_counter()
    raw = raw_ds.get_collate_fn()(raw_items)
    out["collate_raw_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    files = file_ds.get_collate_fn()(file_items)
    out["collate_files_s"] = time.perf_counter() - t0
    raw, files = pin(raw), pin(files)
    out["bus_bytes_raw"], out["bus_bytes_files"] = tensor_bytes(raw), tensor_bytes(files)
    out["png_bytes"], out["annotation_bytes"] = int(files["png_table"][:, 1].sum()), int(files["annotation_table"][:, 1].sum())
    out["decoded_image_bytes"] = int((files["png_table"][:, 2] * files["png_table"][:, 3] * 3).sum())

    builder = FlameBatchBuilder(cfg, 0)
    images_raw, t_raw = builder(raw)
    images_files, t_files = builder(files)
    torch.cuda.synchronize()
    out["fallbacks"] = dict(builder.last_fallbacks)
    out["forms_bit_equal"] = bool(torch.equal(images_raw, images_files) and all(
        torch.equal(t_raw[k], t_files[k]) for k in t_raw if torch.is_tensor(t_raw[k])))
    out["raw_builder_s"] = event_time(lambda: builder(raw), iters, 3)
    out["raw_builder_wall_s"] = host_time(lambda: builder(raw), iters)
    out["files_builder_s"] = host_time(lambda: builder(files), iters)

    # the file form's parts, each alone between events
    up = {k: v.to(dev) for k, v in files.items() if torch.is_tensor(v)}

    def h2d():
        for key, v in files.items():
            if torch.is_tensor(v):
                up[key].copy_(v, non_blocking=True)

    lib, s = builder._lib, torch.cuda.current_stream(dev).cuda_stream
    png_table = files["png_table"].numpy()
    heads = [tuple(int(v) for v in row[2:]) for row in png_table]
    from dad_3dheads_amd.png_reader import PngDecoder

    decoder = PngDecoder(dev)

    def png():
        decoder._launch_packed(up["png_files"], png_table[:, 0], png_table[:, 1], 3, heads=heads)

    n = builder.n_verts
    offsets, sizes = up["annotation_table"][:, 0].contiguous(), up["annotation_table"][:, 1].contiguous()
    verts = torch.empty((b, n, 3), device=dev)
    mv, pm = torch.empty((b, 4, 4), device=dev), torch.empty((b, 4, 4), device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)

    def annotation():
        lib.dad3d_annotation_parse(up["annotations"].data_ptr(), up["annotations"].numel(), offsets.data_ptr(), sizes.data_ptr(), b, n,
                                   verts.data_ptr(), mv.data_ptr(), pm.data_ptr(), status.data_ptr(), 0, s)

    annotation()
    torch.cuda.synchronize()
    assert not status.any().item(), status
    pending = decoder._launch_packed(up["png_files"], png_table[:, 0], png_table[:, 1], 3, heads=heads)
    full_images = pending.finish(*pending.words_on_host()).tensors()
    descs = up["crop_descs"].clone()
    descs[:, 0] += torch.tensor([t.data_ptr() for t in full_images], dtype=torch.int64).to(dev)

    def rest():
        builder._build(files, descs, up["frames"], verts, mv, pm)

    out["files_h2d_s"] = event_time(h2d, iters, 3)
    out["files_png_s"] = event_time(png, iters, 3)
    out["files_annotation_s"] = event_time(annotation, iters, 3)
    out["files_rest_s"] = event_time(rest, iters, 3)
    out["annotation_bound_s"] = (out["annotation_bytes"] + b * (n * 3 + 32) * 4) / HBM_ACHIEVABLE
    out["annotation_gbps"] = out["annotation_bytes"] / out["files_annotation_s"] / 1e9
    out["loader_items_per_s_per_cpu"] = {"raw": 1 / out["getitem_raw_s"], "files": 1 / out["getitem_files_s"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_files_bench.json"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    st = synthetic.load_static()
    iters = 3 if args.quick else 20
    runs = []
    for b in (64, 256):
        with tempfile.TemporaryDirectory() as root:
            runs.append(bench(b, iters, st, root))
    res = {"device": torch.cuda.get_device_name(0), "iters": iters, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "runs": runs}
    print(json.dumps(res, indent=1))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
