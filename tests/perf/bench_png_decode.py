#!/usr/bin/env python3
"""The PNG decoder (dad-3dheads_amd/png_reader.py, csrc/png_decode.hip) on one MI355X beside PIL on one core, in the same process.
Not collected by pytest.

64 files of the fixture photo at 512 x 512 x 3 (the photo mirrored out to that size, each file shifted by one more row so that no
two are equal), in two forms: written by PIL at compress_level 6, and written by `writers.png_batch`. Per form:
  pil_s            `np.asarray(Image.open(f).convert("RGB"))` of all 64 on one core (host clock, best of 3)
  kernels_s        the launches of dad3d_png_decode with the file bytes already on the device (CUDA events, after warm-up)
  with_upload_s    the same plus the copy of the file bytes from pinned memory (CUDA events)
  decode_call_s    `PngDecoder.decode` end to end: read, stage, upload, launch, the flags' sync (host clock, best of 3)
The library's own files are measured on the segmented path and again with the general path forced. Every device result is compared
with PIL before it is timed. The numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_png_decode.py [--out profiles/png_decode_bench.json]
"""
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, png_reader, writers  # noqa: E402
from event_timer import event_time  # noqa: E402

BATCH, SIDE = 64, 512


def photos():
    with np.load(os.path.join(ROOT, "tests", "golden", "demo_image.npz")) as z:
        photo = z["resized"]
    big = np.pad(photo, ((0, 2 * SIDE - photo.shape[0]), (0, 2 * SIDE - photo.shape[1]), (0, 0)), mode="symmetric")
    return np.stack([np.ascontiguousarray(big[i:i + SIDE, i:i + SIDE]) for i in range(BATCH)])


def host_clock(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def pil_decode(files):
    return [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]


class Plan:
    """The buffers of one dad3d_png_decode call, allocated once."""

    def __init__(self, files, force_general):
        self.lib = _lib.load()
        rows, at, out_at = [], 0, 0
        for f in files:
            rows.append([at, len(f), SIDE, SIDE, 3, out_at, SIDE * 3, 3, 0, 0, 0, 0])
            at += (len(f) + 15) // 16 * 16
            out_at += SIDE * SIDE * 3
        desc = np.asarray(rows, dtype=np.int64)
        most = C.c_int32(0)
        self.scratch_bytes = self.lib.dad3d_png_decode_scratch_bytes(desc.ctypes.data, len(rows), C.addressof(most))
        self.most, self.n, self.file_bytes, self.out_bytes, self.force = most.value, len(rows), at, out_at, int(force_general)
        self.pinned = torch.zeros(at, dtype=torch.uint8, pin_memory=True)
        for row, f in zip(rows, files):
            self.pinned.numpy()[row[0]:row[0] + row[1]] = np.frombuffer(f, dtype=np.uint8)
        self.data = self.pinned.cuda()
        self.desc = torch.from_numpy(desc).cuda()
        self.out = torch.empty(out_at, dtype=torch.uint8, device="cuda")
        self.flags = torch.empty(len(rows), dtype=torch.int32, device="cuda")
        self.info = torch.empty(len(rows), dtype=torch.int32, device="cuda")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device="cuda")

    def launch(self):
        _lib.check(self.lib.dad3d_png_decode(self.data.data_ptr(), self.file_bytes, self.desc.data_ptr(), self.n, self.most, self.out.data_ptr(),
                                             self.out_bytes, self.flags.data_ptr(), self.info.data_ptr(), self.scratch.data_ptr(),
                                             self.scratch_bytes, self.force, 0, torch.cuda.current_stream().cuda_stream))

    def upload_and_launch(self):
        self.data.copy_(self.pinned, non_blocking=True)
        self.launch()


def measure(name, files, want, force_general, segmented, iters):
    plan = Plan(files, force_general)
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.flags.cpu().any()
    assert plan.info.cpu().tolist() == [int(segmented)] * len(files)
    got = plan.out.view(len(files), SIDE, SIDE, 3).cpu().numpy()
    assert np.array_equal(got, want)
    decoder = png_reader.PngDecoder(0)
    res = decoder.decode(files, channels=3, force_general=force_general)
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(res.tensors(), want))
    t_kernels = event_time(plan.launch, iters, 3)
    t_upload = event_time(plan.upload_and_launch, iters, 3)
    t_call = host_clock(lambda: decoder.decode(files, channels=3, force_general=force_general), 3)
    return {"form": name, "path": "segmented" if segmented else "general", "file_bytes": sum(map(len, files)), "kernels_s": t_kernels,
            "with_upload_s": t_upload, "decode_call_s": t_call, "images_per_s_kernels": len(files) / t_kernels,
            "images_per_s_with_upload": len(files) / t_upload}


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    images = photos()
    by_pil = []
    for img in images:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG", compress_level=6)
        by_pil.append(buf.getvalue())
    own = [bytes(f) for f in writers.png_batch(torch.from_numpy(images).cuda())]
    runs = []
    for name, files in (("PIL level 6", by_pil), ("png_batch", own)):
        want = np.stack(pil_decode(files))
        assert np.array_equal(want, images)
        t_pil = host_clock(lambda: pil_decode(files), 3)
        legs = [measure(name, files, want, True, False, 5)]
        if files is own:
            legs.append(measure(name, files, want, False, True, 20))
        for leg in legs:
            leg.update(pil_s=t_pil, pil_images_per_s=len(files) / t_pil, speedup_kernels=t_pil / leg["kernels_s"],
                       speedup_with_upload=t_pil / leg["with_upload_s"], speedup_decode_call=t_pil / leg["decode_call_s"])
        runs += legs
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "batch": BATCH, "shape": [SIDE, SIDE, 3],
           "segment_bytes": _lib.PNG_SEGMENT_BYTES, "runs": runs}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
