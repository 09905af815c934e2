#!/usr/bin/env python3
"""`FaceMeshPredictor.predict_boxes` (csrc/preprocess_boxes.hip) on one MI355X beside the route it replaces, in the same process: crops cut
on the host, each uploaded on its own, then `predict_batch`. Not collected by pytest.

`random_init(dtype=torch.bfloat16)` (the DAD-3DNet declaration, seeded weights; the synthetic FLAME model), 8 frames of 1080 x 1920 with 8 boxes each, offset 0.1.
  host_crops_predict_batch_s  the former route: extend_bbox + ensure_bbox_boundaries + slicing on the host, 64 uploads, predict_batch
  predict_boxes_s             host frames and host boxes: 8 uploads, one preprocess launch, results in the frames' coordinates
  predict_boxes_device_s      frames and boxes already on the device (a decoder's and a detector's outputs): no upload, no host wait
  preprocess_*_s              the launches alone (CUDA events): the former launch on the 64 uploaded crops, the cast and layout pass
                              InferenceNet.forward makes of its result, and the new launch in float32 planar and in bf16 channels-last
The end-to-end times are host clocks around calls that end in a synchronise, results left on the device (`device_outputs=True,
points_on_device=True`) on both sides. Every time is the median of five repeats of its loop, the routes alternating inside a repeat;
`*_spread_s` is the largest minus the smallest of the five. `clock_mhz` is the shader clock read before (idle) and after.
`network_input_equal`: the bf16 launch writes the bits the former launch and the cast make; `*_max_abs_diff_*`: the results of the two
routes beside the former route run twice. The numbers are
recorded as measured; no condition is asserted on them.

    python tests/perf/bench_predict_boxes.py [--out profiles/predict_boxes_bench.json]
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
from dad_3dheads_amd import _lib, synthetic  # noqa: E402
from dad_3dheads_amd.dataset import ensure_bbox_boundaries, extend_bbox  # noqa: E402
from dad_3dheads_amd.predictor import FaceMeshPredictor  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W = 8, 8, 1080, 1920


def host_time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception as e:  # no management library: say so
        return f"not read ({type(e).__name__})"


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 10
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(FRAMES)]
    boxes = []
    for _ in range(FRAMES):  # heads of 120 .. 500 pixels, some over the frame's edges
        wh = rng.integers(120, 500, (PER_FRAME, 2))
        xy = np.stack([rng.integers(-40, W - 100, PER_FRAME), rng.integers(-40, H - 100, PER_FRAME)], axis=1)
        boxes.append(np.concatenate([xy, wh], axis=1).astype(np.int32))
    pred = FaceMeshPredictor.random_init(dtype=torch.bfloat16, flame_model=synthetic.synthetic_flame_model(0, synthetic.load_static()))
    flags = dict(device_outputs=True, points_on_device=True)

    def former():
        crops = []
        for f, bs in zip(frames, boxes):
            for b in bs:
                x, y, w, h = ensure_bbox_boundaries(extend_bbox(b, 0.1), f.shape[:2])
                crops.append(f[y:y + h, x:x + w])
        return pred.predict_batch(crops, **flags), crops

    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    d_boxes = torch.from_numpy(np.concatenate(boxes)).cuda()
    d_index = torch.arange(FRAMES, dtype=torch.int32).repeat_interleave(PER_FRAME).cuda()
    routes = {"host_crops_predict_batch_s": lambda: former(),
              "predict_boxes_s": lambda: pred.predict_boxes(frames, boxes, **flags),
              "predict_boxes_device_s": lambda: pred.predict_boxes(d_frames, d_boxes, d_index, **flags)}
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W],
           "boxes": FRAMES * PER_FRAME, "dtype": "bfloat16", "iters": iters, "clock_mhz": [clock_mhz()]}
    for fn in routes.values():  # warm-up: MIOpen picks its kernels for the batch of 64
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # same inputs to the network, and the former results moved into the frames
    old, crops = former()
    new = pred.predict_boxes(frames, boxes, **flags)
    staged = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in crops]
    sources = [(t.data_ptr(), t.shape[0], t.shape[1], t.shape[1] * 3) for t in staged]
    x_old = pred._preprocess_launch(sources).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x_new = pred._preprocess_boxes_launch(d_frames, d_boxes, d_index, (0.1,) * 4, _lib.PREPROCESS_OUT_BF16_NHWC)[0]
    res["network_input_equal"] = bool(torch.equal(x_old, x_new))
    # the network's own run-to-run spread on one input (its convolutions may sum in any order) beside the difference between the routes
    again = former()[0]
    res["vertices_3d_max_abs_diff_former_twice"] = max(float((a["3d_vertices"] - b["3d_vertices"]).abs().max()) for a, b in zip(old, again))
    res["vertices_3d_max_abs_diff_routes"] = max(float((a["3d_vertices"] - b["3d_vertices"]).abs().max()) for a, b in zip(old, new))
    res["points_max_abs_diff_routes"] = max(int((a["points"] + b["bbox"][:2] - b["points"]).abs().max()) for a, b in zip(old, new))

    times = {k: [] for k in routes}
    for _ in range(5):
        for k, fn in routes.items():
            times[k].append(host_time(fn, iters))
    for k, v in times.items():
        v.sort()
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
    f32 = pred._preprocess_launch(sources)
    launches = {"preprocess_images_s": lambda: pred._preprocess_launch(sources),
                "cast_and_layout_s": lambda: f32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last),
                "preprocess_boxes_f32_s": lambda: pred._preprocess_boxes_launch(d_frames, d_boxes, d_index, (0.1,) * 4, _lib.PREPROCESS_OUT_F32_NCHW),
                "preprocess_boxes_bf16_s": lambda: pred._preprocess_boxes_launch(d_frames, d_boxes, d_index, (0.1,) * 4, _lib.PREPROCESS_OUT_BF16_NHWC)}
    for k, fn in launches.items():  # each includes its table's upload and its output's allocation, as a call does
        v = sorted(event_time(fn, 200, 10) for _ in range(5))
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
    res["clock_mhz"].append(clock_mhz())
    res["speedup_host_boxes"] = res["host_crops_predict_batch_s"] / res["predict_boxes_s"]
    res["speedup_device_boxes"] = res["host_crops_predict_batch_s"] / res["predict_boxes_device_s"]
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
