#!/usr/bin/env python3
"""`tracking.HeadTracker.step` with `steady` and `merge_iou` (csrc/track_steady.hip) on one MI355X beside the same step with both off,
in the same process. Not collected by pytest.

The set-up of bench_track.py: `random_init(dtype=torch.bfloat16)` (the DAD-3DNet declaration, seeded weights; the synthetic FLAME
model), 8 frames of 1080 x 1920 already on the device with 8 heads each, T = 20 steps of a loop, offset 0.1, and a slot that is
flagged gets its starting box again after every step on the device, so that all 64 slots stay at work in both modes.
  off_loop_s   T x `HeadTracker(pred).step`; one synchronise after the last step. `off_loop_per_step_s` beside
               `parent_per_step_s` (the 7.93 ms a step profiles/track_bench.json records for the commit before the options
               existed) says whether the "off" mode has moved
  on_loop_s    the same with `HeadTracker(pred, steady=SteadyConfig(), merge_iou=0.5)`: one filter launch, one `[64,413]` copy
               (`3dmm_params_raw`) and one suppress launch more a step
Loop times are host clocks around T steps ending in a synchronise; every time is the median of five repeats, the two modes
alternating inside a repeat; `*_spread_s` is the largest minus the smallest of the five. `on_minus_off_per_step_s` is the
difference of the medians. `duplicates_per_step` and `lost_per_step` are the last "on" run's counts. In the recorded run both are 0 at
every step: the seeded network's 64 heads stayed in their frames and apart, so the loop timed the two launches but never a slot being
zeroed (the kernels' cost barely depends on that; `suppress_s` below runs on the overlapping starting boxes).
Each launch alone (CUDA events around 200 calls, medians of five), beside a torch chain on the device that does less:
  one_euro_rows_s          the filter launch on `[64,413]`, in place
  one_euro_torch_chain_s   rule 4 alone as torch elementwise operations on the same tensors -- no flags, no row-wide test for a
                           NaN or an overflow, no ages
  suppress_s, suppress_cap_s       the suppress launch on 64 and on 1024 slots (boxes restored by a copy that is part of the time)
  suppress_torch_chain_s           the pairwise IoU matrix of the 64 boxes and "overlaps any earlier slot", which is not the greedy rule
`clock_mhz` is the shader clock read before (idle) and after. The numbers are recorded as measured; no condition is asserted.

    python tests/perf/bench_track_steady.py [--out profiles/track_steady_bench.json]
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
from dad_3dheads_amd import _lib, boxes as host_boxes, steady, synthetic  # noqa: E402
from dad_3dheads_amd.predictor import FaceMeshPredictor  # noqa: E402
from dad_3dheads_amd.tracking import HeadTracker  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W, STEPS = 8, 8, 1080, 1920, 20
PARENT_PER_STEP_S = 0.007929202751256526  # profiles/track_bench.json: device_loop_per_step_s


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
    start = []
    for _ in range(FRAMES):  # heads of 120 .. 500 pixels inside their frames
        wh = rng.integers(120, 500, (PER_FRAME, 2))
        xy = np.stack([rng.integers(0, W - 500, PER_FRAME), rng.integers(0, H - 500, PER_FRAME)], axis=1)
        start.append(np.concatenate([xy, wh], axis=1).astype(np.int32))
    flat, index = host_boxes.flatten_boxes(FRAMES, start)
    d_start, d_index = torch.from_numpy(flat).cuda(), torch.from_numpy(index).cuda()
    slots = torch.arange(len(flat), device="cuda")
    pred = FaceMeshPredictor.random_init(dtype=torch.bfloat16, flame_model=synthetic.synthetic_flame_model(0, synthetic.load_static()))
    trackers = {"off_loop_s": HeadTracker(pred), "on_loop_s": HeadTracker(pred, steady=steady.SteadyConfig(), merge_iou=0.5)}
    lost_log = []

    def loop(tracker):
        tracker.start(d_frames, d_start, d_index)
        lost_log.clear()
        for _ in range(steps):
            tracker.step(d_frames)
            lost = tracker.lost()
            lost_log.append(lost.clone())
            tracker.reseed(slots, torch.where(lost[:, None] != 0, d_start, tracker.boxes()))
        torch.cuda.synchronize()

    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W],
           "heads": FRAMES * PER_FRAME, "steps": steps, "dtype": "bfloat16", "clock_mhz": [clock_mhz()], "parent_per_step_s": PARENT_PER_STEP_S}
    for tracker in trackers.values():  # warm-up: MIOpen picks its kernels for the batch of 64
        loop(tracker)
    times = {k: [] for k in trackers}
    for _ in range(5):
        for k, tracker in trackers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(tracker)
            times[k].append(time.perf_counter() - t0)
    res["lost_per_step"] = [int((t != 0).sum()) for t in lost_log]  # the last run was an "on" run
    res["duplicates_per_step"] = [int((t == _lib.TRACK_FLAG_DUPLICATE).sum()) for t in lost_log]
    for k, v in times.items():
        v.sort()
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
        res[k[:-2] + "_per_step_s"] = v[2] / steps
    res["on_minus_off_per_step_s"] = res["on_loop_per_step_s"] - res["off_loop_per_step_s"]
    res["off_over_parent"] = res["off_loop_per_step_s"] / PARENT_PER_STEP_S

    # each launch alone, beside a torch chain that does less
    n, d = len(flat), 413
    cfg = steady.SteadyConfig()
    min_cutoff, beta = (torch.from_numpy(v).cuda() for v in cfg.expand())
    filt = steady.OneEuroFilter(n, d, min_cutoff.cpu().numpy(), beta.cpu().numpy(), cfg.d_cutoff, "cuda:0")
    x = torch.from_numpy(rng.normal(0.0, 1.0, (n, d)).astype(np.float32)).cuda()
    work, zero_flags = x.clone(), torch.zeros(n, dtype=torch.int32, device="cuda")
    rate, two_pi_dt, alpha_d = (float(s) for s in steady.one_euro_scalars(cfg.dt, cfg.d_cutoff))
    filt.step(x, zero_flags, cfg.dt)  # the first sample: what is timed is rule 4
    state_x, state_dx = filt.state_x.clone(), filt.state_dx.clone()

    def euro_chain():
        dx = (work - state_x) * rate
        dxh = state_dx + alpha_d * (dx - state_dx)
        r = two_pi_dt * (min_cutoff + beta * dxh.abs())
        o = state_x + r / (r + 1.0) * (work - state_x)
        state_x.copy_(o)
        state_dx.copy_(dxh)
        return o

    many = np.concatenate([flat + np.array([k * 7, k * 5, 0, 0], np.int32) for k in range(_lib.TRACK_MAX_SLOTS // n)])
    d_many, many_index = torch.from_numpy(many).cuda(), d_index.repeat(_lib.TRACK_MAX_SLOTS // n)
    work_boxes, work_flags = d_start.clone(), torch.zeros(n, dtype=torch.int32, device="cuda")
    cap_boxes, cap_flags = d_many.clone(), torch.zeros(len(many), dtype=torch.int32, device="cuda")

    def suppress(boxes_now, flags_now, source, image_index):
        boxes_now.copy_(source)
        flags_now.zero_()
        pred._suppress_duplicates_launch(boxes_now, flags_now, image_index, 0.5)

    def suppress_chain():
        b = d_start.to(torch.int64)
        x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
        iw = (torch.minimum(x1[:, None], x1[None]) - torch.maximum(x0[:, None], x0[None])).clamp(min=0)
        ih = (torch.minimum(y1[:, None], y1[None]) - torch.maximum(y0[:, None], y0[None])).clamp(min=0)
        inter = iw * ih
        area = b[:, 2] * b[:, 3]
        hit = (inter > 0) & (inter.double() >= 0.5 * (area[:, None] + area[None] - inter).double()) & (d_index[:, None] == d_index[None])
        return torch.triu(hit, diagonal=1).any(dim=0)

    launches = {"one_euro_rows_s": lambda: filt.step(work, zero_flags, cfg.dt, out=work), "one_euro_torch_chain_s": euro_chain,
                "suppress_s": lambda: suppress(work_boxes, work_flags, d_start, d_index),
                "suppress_cap_s": lambda: suppress(cap_boxes, cap_flags, d_many, many_index), "suppress_torch_chain_s": suppress_chain}
    for k, fn in launches.items():
        v = sorted(event_time(fn, 200, 10) for _ in range(5))
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
    res["restore_copy_s"] = sorted(event_time(lambda: (work_boxes.copy_(d_start), work_flags.zero_()), 200, 10) for _ in range(5))[2]
    res["clock_mhz"].append(clock_mhz())
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
