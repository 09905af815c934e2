#!/usr/bin/env python3
"""The JPEG encoder (writers.JpegEncoder, csrc/jpeg_encode.hip) on one MI355X beside PIL on one core, in the same process. Not
collected by pytest.

64 images of the fixture photo at 512 x 512 x 3 (the photo mirrored out to that size, each image shifted by one more row so that no
two are equal), quality 75, 4:2:0, in two forms: without restart markers and with `restart_marker_rows=1` (32 intervals per file).
Per form:
  pil_s            `Image.fromarray(img).save(buf, "JPEG", ..)` of all 64 on one core (host clock, best of 3)
  kernels_s        the two launches of dad3d_jpeg_encode with the pixels resident on the device (device events, after warm-up)
  encode_call_s    `JpegEncoder.encode(..).to_host()` end to end: launch, the lengths' sync, the copy of the files (host clock, best of 3)
  bytes_per_image  the mean file size, beside `png_bytes_per_image` of `PngEncoder` on the same pixels
  decode_kernels_s the launches of dad3d_jpeg_decode on the files just written (device events), beside `pil_decode_s`
Every device file is compared with PIL's before anything is timed. The numbers are recorded as measured; no condition is asserted.

    python tests/perf/bench_jpeg_encode.py [--out profiles/jpeg_encode_bench.json]
"""
import io
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from dad_3dheads_amd import _lib, writers  # noqa: E402
from bench_jpeg_decode import BATCH, SIDE, Plan, host_clock, photos, pil_decode  # noqa: E402
from event_timer import event_time  # noqa: E402

QUALITY, SUBSAMPLING = 75, 2


def pil_encode(images, rows):
    files = []
    for img in images:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING, restart_marker_rows=rows)
        files.append(buf.getvalue())
    return files


def measure(name, rows, images, pixels, png_bytes, iters):
    enc = writers.JpegEncoder(SIDE, SIDE, 3, quality=QUALITY, subsampling=SUBSAMPLING, restart_marker_rows=rows, device=0)
    enc.reserve(BATCH)
    want = pil_encode(images, rows)
    data = enc.encode(pixels)
    files = [bytes(x) for x in data.to_host()]
    assert not data.flags.cpu().any() and files == want
    t_pil = host_clock(lambda: pil_encode(images, rows), 3)
    t_kernels = event_time(lambda: enc.encode(pixels), iters, 3)
    t_call = host_clock(lambda: enc.encode(pixels).to_host(), 3)
    plan = Plan(files)
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.flags.cpu().any()
    assert np.array_equal(plan.out.view(BATCH, SIDE, SIDE, 3).cpu().numpy(), np.stack(pil_decode(files)))
    t_decode = event_time(plan.launch, 5, 2)
    t_pil_decode = host_clock(lambda: pil_decode(files), 3)
    total = sum(map(len, files))
    return {"form": name, "restart_interval_mcus": enc.restart_interval, "pil_s": t_pil, "pil_images_per_s": BATCH / t_pil,
            "kernels_s": t_kernels, "images_per_s_kernels": BATCH / t_kernels, "pixel_bytes_per_s_kernels": pixels.numel() / t_kernels,
            "speedup_kernels": t_pil / t_kernels, "encode_call_s": t_call, "speedup_encode_call": t_pil / t_call,
            "bytes_per_image": total / BATCH, "png_bytes_per_image": png_bytes / BATCH, "file_row_bytes": enc.stride,
            "decode_kernels_s": t_decode, "pil_decode_s": t_pil_decode, "speedup_decode_kernels": t_pil_decode / t_decode}


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    images = photos()
    pixels = torch.from_numpy(images).cuda()
    png = writers.PngEncoder(SIDE, SIDE, 3, device=0).encode(pixels)
    torch.cuda.synchronize()
    assert not png.flags.cpu().any()
    png_bytes = int(png.lengths.sum())
    runs = [measure(name, rows, images, pixels, png_bytes, 20) for name, rows in (("no restart markers", 0), ("restart_marker_rows=1", 1))]
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "batch": BATCH, "shape": [SIDE, SIDE, 3],
           "quality": QUALITY, "subsampling": "4:2:0", "runs": runs}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
