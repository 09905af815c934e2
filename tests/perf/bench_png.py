#!/usr/bin/env python3
"""The PNG encoder (dad-3dheads_amd/writers.py `PngEncoder`, csrc/png_encode.hip) on one MI355X beside PIL on the copied-back
array, in the same process. Not collected by pytest.

Batches of 64 and 1024 images of 256 x 256 x 3: the golden head render, PNCC map, UV texture and photo crop in turn (the photo
padded to 256 columns with its edge), so the batch holds smooth renders and a noisy photograph alike. Per batch:
  encode_kernels_s     the three launches of `PngEncoder.encode` (CUDA events, after warm-up)
  copy_to_pinned_s     lengths + flags, the dense repack and the copy of the files into pinned memory (host clock, synchronised)
  save_png_batch_s     `save_png_batch` of the CUDA batch end to end: encode, copy, one file per image written (host clock)
  pixels_to_host_s     the copy of the pixels the host path starts with
  pil_level1_s / pil_default_s   `PIL.Image.save(format="PNG", compress_level=1 / default)` of every image of the copied-back
                       array into memory (host clock, one run)
  file_bytes, pil_level1_bytes, pil_default_bytes   the sizes of what each wrote
Every device file is decoded with PIL and compared with the input before anything is timed. The numbers are recorded as
measured; no condition is asserted on them.

    python tests/perf/bench_png.py [--out profiles/png_bench.json]
"""
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, writers  # noqa: E402
from event_timer import event_time  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def source_images():
    with np.load(os.path.join(GOLDEN, "sim3dr_golden.npz")) as z:
        head, pncc = z["head_image"], z["pncc_image"]
    with np.load(os.path.join(GOLDEN, "uv_texture_golden.npz")) as z:
        texture = z["textures"][0]
    with np.load(os.path.join(GOLDEN, "demo_image.npz")) as z:
        photo = z["resized"]
    photo = np.pad(photo, ((0, 0), (0, 256 - photo.shape[1]), (0, 0)), mode="edge")
    return [np.ascontiguousarray(x) for x in (head, pncc, texture, photo)]


def host_clock(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def pil_batch(arr, **kwargs):
    out = []
    for a in arr:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG", **kwargs)
        out.append(buf.getvalue())
    return out


def measure(batch, iters):
    src = source_images()
    host = np.stack([src[i % len(src)] for i in range(batch)])
    images = torch.from_numpy(host).cuda()
    enc = writers.PngEncoder(256, 256, 3, device=0)
    enc.reserve(batch)
    data = enc.encode(images)
    torch.cuda.synchronize()
    assert not data.flags.cpu().any()
    files = [bytes(x) for x in data.to_host()]
    for i in range(min(batch, 8)):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[i]))), host[i]), i
    assert all(files[i] == files[i % len(src)] for i in range(batch))

    t_kernels = event_time(lambda: enc.encode(images), iters, 3)

    def copy():
        data._copy = None
        data.begin_host_copy()
        data._copy[3].synchronize()

    copy()
    t_copy = host_clock(copy, 3)
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"{i}.png") for i in range(batch)]
        writers.save_png_batch(images, paths)
        t_save = host_clock(lambda: writers.save_png_batch(images, paths), 2)
    back = []
    t_pixels = host_clock(lambda: back.append(images.cpu().numpy()), 2)
    level1, default = [], []
    t_l1 = host_clock(lambda: level1.append(pil_batch(back[-1], compress_level=1)), 1)
    t_def = host_clock(lambda: default.append(pil_batch(back[-1])), 1)
    return {"B": batch, "shape": [256, 256, 3], "encode_kernels_s": t_kernels, "copy_to_pinned_s": t_copy, "device_s": t_kernels + t_copy,
            "save_png_batch_s": t_save, "pixels_to_host_s": t_pixels, "pil_level1_s": t_l1, "pil_default_s": t_def,
            "file_bytes": sum(map(len, files)), "pil_level1_bytes": sum(map(len, level1[0])), "pil_default_bytes": sum(map(len, default[0])),
            "speedup_vs_pil_level1": (t_pixels + t_l1) / (t_kernels + t_copy), "speedup_vs_pil_default": (t_pixels + t_def) / (t_kernels + t_copy)}


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
           "segment_bytes": _lib.PNG_SEGMENT_BYTES, "runs": [measure(64, iters=20), measure(1024, iters=5)]}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
