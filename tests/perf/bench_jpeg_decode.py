#!/usr/bin/env python3
"""The JPEG decoder (dad-3dheads_amd/jpeg_reader.py, csrc/jpeg_decode.hip) on one MI355X beside PIL on one core, in the same
process. Not collected by pytest.

64 files of the fixture photo at 512 x 512 x 3 (the photo mirrored out to that size, each file shifted by one more row so that no
two are equal), written by PIL at 4:2:0 and quality 90, in two forms: without restart markers (one entropy segment, so one lane, per
file: the 64 files share one wave) and with `restart_marker_rows=1` (32 segments per file). Per form:
  pil_s            `np.asarray(Image.open(f).convert("RGB"))` of all 64 on one core (host clock, best of 3)
  kernels_s        the launches of dad3d_jpeg_decode with the file bytes already on the device (CUDA events, after warm-up)
  with_upload_s    the same plus the copy of the file bytes from pinned memory (CUDA events)
  decode_call_s    `JpegDecoder.decode` end to end: read, stage, upload, launch, the flags' sync (host clock, best of 3)
  predict_files_s / predict_batch_pil_s   `FaceMeshPredictor.predict_files` on the files beside PIL's decode followed by
                   `predict_batch` on its arrays, with a model of a few operations so that the decode shows (host clock, best of 3)
Every device result is compared with PIL before it is timed. The numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_jpeg_decode.py [--out profiles/jpeg_decode_bench.json]
"""
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
from dad_3dheads_amd import _lib, jpeg_reader, synthetic  # noqa: E402
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
    """The buffers of one dad3d_jpeg_decode call, allocated once."""

    def __init__(self, files):
        self.lib = _lib.load()
        rows, at, out_at = [], 0, 0
        for f in files:
            rows.append([at, len(f), SIDE, SIDE, 3, out_at, SIDE * 3, 3, 0, 0, 0, 0])
            at += (len(f) + 15) // 16 * 16
            out_at += SIDE * SIDE * 3
        desc = np.asarray(rows, dtype=np.int64)
        self.grid = np.zeros(_lib.JPEG_DECODE_GRID_INTS, dtype=np.int32)
        self.scratch_bytes = self.lib.dad3d_jpeg_decode_scratch_bytes(desc.ctypes.data, len(rows), self.grid.ctypes.data)
        self.n, self.file_bytes, self.out_bytes = len(rows), at, out_at
        self.pinned = torch.zeros(at, dtype=torch.uint8, pin_memory=True)
        for row, f in zip(rows, files):
            self.pinned.numpy()[row[0]:row[0] + row[1]] = np.frombuffer(f, dtype=np.uint8)
        self.data = self.pinned.cuda()
        self.desc = torch.from_numpy(desc).cuda()
        self.out = torch.empty(out_at, dtype=torch.uint8, device="cuda")
        self.flags = torch.empty(len(rows), dtype=torch.int32, device="cuda")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device="cuda")

    def launch(self):
        _lib.check(self.lib.dad3d_jpeg_decode(self.data.data_ptr(), self.file_bytes, self.desc.data_ptr(), self.n, self.grid.ctypes.data,
                                              self.out.data_ptr(), self.out_bytes, self.flags.data_ptr(), self.scratch.data_ptr(),
                                              self.scratch_bytes, 0, torch.cuda.current_stream().cuda_stream))

    def upload_and_launch(self):
        self.data.copy_(self.pinned, non_blocking=True)
        self.launch()


class Small(torch.nn.Module):
    """A model of a few operations: parameters and landmarks moved by the mean colour of the input."""

    def __init__(self):
        super().__init__()
        self.register_buffer("base", torch.from_numpy(synthetic.synthetic_params(1, seed=8))[0])
        self.register_buffer("ramp", torch.linspace(0.2, 0.9, 68)[None, :, None])

    def forward(self, x):
        feat = x.float().mean(dim=(2, 3))
        p = self.base[None] + 0.01 * torch.tanh(feat).sum(1, keepdim=True)
        lm = torch.sigmoid(feat[:, :2])[:, None, :].expand(-1, 68, -1) * self.ramp
        return {"OUTPUT_3DMM_PARAMS": p, "OUTPUT_2D_LANDMARKS": lm}


def measure(name, files, want, predictor, iters):
    plan = Plan(files)
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.flags.cpu().any()
    assert np.array_equal(plan.out.view(len(files), SIDE, SIDE, 3).cpu().numpy(), want)
    decoder = jpeg_reader.JpegDecoder(0)
    res = decoder.decode(files, channels=3)
    assert not res.flags.any() and all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(res.tensors(), want))
    by_files, by_pil = predictor.predict_files(files), predictor.predict_batch(pil_decode(files))
    assert all(torch.equal(a["3dmm_params"], b["3dmm_params"]) and np.array_equal(a["points"], b["points"]) for a, b in zip(by_files, by_pil))
    t_pil = host_clock(lambda: pil_decode(files), 3)
    t_kernels = event_time(plan.launch, iters, 2)
    t_upload = event_time(plan.upload_and_launch, iters, 2)
    t_call = host_clock(lambda: decoder.decode(files, channels=3), 3)
    t_files = host_clock(lambda: predictor.predict_files(files), 3)
    t_batch = host_clock(lambda: predictor.predict_batch(pil_decode(files)), 3)
    return {"form": name, "file_bytes": sum(map(len, files)), "segments_per_file": 1 + sum(files[0].count(bytes([0xFF, 0xD0 + k])) for k in range(8)),
            "pil_s": t_pil, "pil_images_per_s": len(files) / t_pil, "kernels_s": t_kernels, "with_upload_s": t_upload, "decode_call_s": t_call,
            "images_per_s_kernels": len(files) / t_kernels, "speedup_kernels": t_pil / t_kernels, "speedup_with_upload": t_pil / t_upload,
            "speedup_decode_call": t_pil / t_call, "predict_files_s": t_files, "predict_batch_pil_s": t_batch,
            "speedup_predict_files": t_batch / t_files}


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    from dad_3dheads_amd.config import load_default_config
    from dad_3dheads_amd.predictor import FaceMeshPredictor

    predictor = FaceMeshPredictor(load_default_config(), cuda_id=0, model=Small(), flame_model=synthetic.synthetic_flame_model(0, synthetic.load_static()))
    images = photos()
    runs = []
    for name, options in (("no restart markers", {}), ("restart_marker_rows=1", {"restart_marker_rows": 1})):
        files = []
        for img in images:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=90, subsampling=2, **options)
            files.append(buf.getvalue())
        want = np.stack(pil_decode(files))
        runs.append(measure(name, files, want, predictor, 5))
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "batch": BATCH, "shape": [SIDE, SIDE, 3],
           "quality": 90, "subsampling": "4:2:0", "runs": runs}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
