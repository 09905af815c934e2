#!/usr/bin/env python3
"""`tracking.HeadTracker.step` (csrc/track_boxes.hip) on one MI355X beside the same loop with the boxes taken on the host, in the same
process. Not collected by pytest.

`random_init(dtype=torch.bfloat16)` (the DAD-3DNet declaration, seeded weights; the synthetic FLAME model), 8 frames of 1080 x 1920
already on the device with 8 heads each, T = 20 steps of a loop, offset 0.1, the defaults min_side = 1 and min_visible = 0.5.
  device_loop_s   T x `HeadTracker.step`: predict_boxes on the boxes held on the device, one launch to the next boxes; one
                  synchronise after the last step
  host_loop_s     T x (`predict_boxes(.., device_outputs=False)` with host boxes, numpy `boxes.next_boxes` on the copied
                  `projected_vertices`, host boxes back in): what a caller writes without the tracker
A seeded network's heads are not heads: many leave their frames. So that both loops keep all 64 slots at work, a slot that is
flagged gets its starting box again after every step, on the device (`reseed` with a `torch.where`, no wait) and on the host
alike; `lost_per_step` is how many that were, step by step, in the device loop's last run.
  boxes_from_heads_s   the launch alone (CUDA events) on the 64 heads' `[64,5023,2]`, outputs allocated once
  torch_chain_s        `amin` / `amax` over the vertices, `floor` / `ceil`, the subtraction and the stack on the device: the bounds
                       alone, with no flag, no frame and no zeroing -- less than the kernel does
Loop times are host clocks around T steps ending in a synchronise; every time is the median of five repeats, the routes alternating
inside a repeat; `*_spread_s` is the largest minus the smallest of the five. `clock_mhz` is the shader clock read before (idle) and
after. `final_boxes_equal`: whether the two loops hold the same boxes after their T steps (the bf16 convolutions may sum in any
order from run to run, so this is recorded, not required). The numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_track.py [--out profiles/track_bench.json]
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
from dad_3dheads_amd import _lib, boxes as host_boxes, synthetic  # noqa: E402
from dad_3dheads_amd.predictor import FaceMeshPredictor  # noqa: E402
from dad_3dheads_amd.tracking import HeadTracker  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W, STEPS = 8, 8, 1080, 1920, 20


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception as e:  # no management library: say so
        return f"not read ({type(e).__name__})"


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else STEPS
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    d_frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(FRAMES)]
    shapes = [(H, W)] * FRAMES
    start = []
    for _ in range(FRAMES):  # heads of 120 .. 500 pixels inside their frames
        wh = rng.integers(120, 500, (PER_FRAME, 2))
        xy = np.stack([rng.integers(0, W - 500, PER_FRAME), rng.integers(0, H - 500, PER_FRAME)], axis=1)
        start.append(np.concatenate([xy, wh], axis=1).astype(np.int32))
    flat, index = host_boxes.flatten_boxes(FRAMES, start)
    d_start, d_index = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    slots = torch.arange(len(flat), device="cuda")
    pred = FaceMeshPredictor.random_init(dtype=torch.bfloat16, flame_model=synthetic.synthetic_flame_model(0, synthetic.load_static()))
    tracker = HeadTracker(pred)
    lost_log = []

    def device_loop():
        tracker.start(d_frames, d_start, d_index)
        lost_log.clear()
        for _ in range(steps):
            tracker.step(d_frames)
            lost = tracker.lost()
            lost_log.append(lost.clone())
            tracker.reseed(slots, torch.where(lost[:, None] != 0, d_start, tracker.boxes()))
        torch.cuda.synchronize()
        return tracker.boxes().cpu().numpy()

    def host_loop():
        cur = flat
        for _ in range(steps):
            res = pred.predict_boxes(d_frames, cur, image_index=index)
            proj = np.concatenate([r["projected_vertices"].numpy() for r in res])
            cur, lost = host_boxes.next_boxes(proj, shapes, index, prev_flags=[r["flags"] for r in res])
            cur[lost != 0] = flat[lost != 0]
        torch.cuda.synchronize()
        return cur

    routes = {"device_loop_s": device_loop, "host_loop_s": host_loop}
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W],
           "heads": FRAMES * PER_FRAME, "steps": steps, "dtype": "bfloat16", "clock_mhz": [clock_mhz()]}
    for fn in routes.values():  # warm-up: MIOpen picks its kernels for the batch of 64
        fn()
    res["final_boxes_equal"] = bool(np.array_equal(device_loop(), host_loop()))
    res["lost_per_step"] = [int((t != 0).sum()) for t in lost_log]
    times = {k: [] for k in routes}
    for _ in range(5):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    for k, v in times.items():
        v.sort()
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
        res[k[:-2] + "_per_step_s"] = v[2] / steps
    # the launch alone beside the torch chain that gives the bounds alone
    proj = pred._predict_boxes_batched(d_frames, d_start, d_index, (0.1,) * 4)["projected_vertices"]
    table = pred._frames_table(d_frames)
    out_boxes = torch.empty((len(flat), 4), dtype=torch.int32, device="cuda")
    out_flags = torch.empty(len(flat), dtype=torch.int32, device="cuda")

    def chain():
        lo, hi = torch.floor(proj.amin(dim=1)).to(torch.int32), torch.ceil(proj.amax(dim=1)).to(torch.int32)
        return torch.cat([lo, hi - lo], dim=1)

    launches = {"boxes_from_heads_s": lambda: pred._boxes_from_heads_launch(proj, table, d_index, None, None, 0, 0.0, out_boxes, out_flags),
                "torch_chain_s": chain}
    for k, fn in launches.items():
        v = sorted(event_time(fn, 200, 10) for _ in range(5))
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
    launches["boxes_from_heads_s"]()
    res["kernel_equals_chain"] = bool(torch.equal(out_boxes, chain())) and not bool(out_flags.any())  # min_side 0, min_visible 0: bounds alone
    res["clock_mhz"].append(clock_mhz())
    res["loop_speedup"] = res["host_loop_s"] / res["device_loop_s"]
    res["launch_speedup"] = res["torch_chain_s"] / res["boxes_from_heads_s"]
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
