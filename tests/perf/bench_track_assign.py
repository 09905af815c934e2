#!/usr/bin/env python3
"""`dad3d_track_assign_detections` (csrc/track_assign.hip) and `tracking.HeadTracker.update` on one MI355X. Not collected by pytest.

The launch alone (CUDA events, medians of five repeats, `*_spread_s` the largest minus the smallest of the five; the slot state is
restored by device copies that are part of the time, `restore_*_s` is that copy alone):
  assign_64_s            64 slots x 64 detections: the 64 starting boxes of the loop below as slots (every fourth one free), the same
                         boxes moved by a few pixels as detections
  assign_cap_random_s    1024 x 1024 random boxes of 20 .. 60 pixels over 8 frames of 1080 x 1920
  assign_cap_identical_s 1024 x 1024, every box identical in one frame: min(n, m) = 1024 rounds, the most the kernel runs; every look
                         stops at its first candidate (the ratio 1)
  assign_cap_nested_s    1024 x 1024, every detection the same box and slot k a box that contains it, a little larger with k: 1024
                         rounds again, and in every round every remaining lane looks through everything that is left -- the most
                         work the kernel does
The loop, in the set-up of bench_track_steady.py: `random_init(dtype=torch.bfloat16)`, 8 frames of 1080 x 1920 on the device, 64 heads,
96 slots, T = 20 steps, offset 0.1; the "detector" returns the 64 starting boxes at every step, so a head that drifted is matched
while it overlaps, and spawned again into a free slot when it does not. Host clocks around T steps ending in a synchronise, medians
of five, the modes alternating inside a repeat:
  step_only_loop_s    T x `step` of a tracker started as ever (64 slots, no spare ones, never updated): `step_only_per_step_s` stands
                      beside `parent_per_step_s` if `--parent-per-step` gives the same loop's time on the parent commit, measured on
                      the same machine
  spare_loop_s        T x `step` with the 96 slots and no `update`: the 32 spare slots are lost, but they are rows of every batch
  device_loop_s       T x (`step`, `update` on device tensors): no host read
  host_loop_s         T x (`step`; `lost()`, `boxes()` to the host; `boxes.assign_detections` in numpy; `reseed` of the spawned slots):
                      what a caller had before
`clock_mhz` is the shader clock read before (idle) and after. The numbers are recorded as measured; no condition is asserted.

    python tests/perf/bench_track_assign.py [--out profiles/track_assign_bench.json] [--parent-per-step SECONDS]
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

FRAMES, PER_FRAME, H, W, STEPS, SLOTS = 8, 8, 1080, 1920, 20, 96
MATCH_IOU, MAX_MISSES = 0.3, 5
CAP = _lib.TRACK_MAX_SLOTS


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(0))
    except Exception as e:  # no management library: say so
        return f"not read ({type(e).__name__})"


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else STEPS
    parent = float(argv[argv.index("--parent-per-step") + 1]) if "--parent-per-step" in argv else None
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
    d_count = torch.tensor([len(flat)], dtype=torch.int32, device="cuda")
    pred = FaceMeshPredictor.random_init(dtype=torch.bfloat16, flame_model=synthetic.synthetic_flame_model(0, synthetic.load_static()))
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W],
           "heads": FRAMES * PER_FRAME, "slots": SLOTS, "steps": steps, "dtype": "bfloat16", "match_iou": MATCH_IOU, "max_misses": MAX_MISSES,
           "clock_mhz": [clock_mhz()], "parent_per_step_s": parent}

    # ---- the launch alone ----
    def case(slots, flags, frames_of, dets, det_frames, n_frames, iters):
        state = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (slots, flags, frames_of, np.zeros(len(slots), np.int32))]
        work = [t.clone() for t in state]
        d_dets, d_det_frames = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (dets, det_frames))

        def restore():
            for w, s in zip(work, state):
                w.copy_(s)

        def launch():
            restore()
            return pred.assign_detections(*work, d_dets, d_det_frames, n_frames, MATCH_IOU, max_misses=MAX_MISSES)

        assign, det_flags, spawned = launch()
        torch.cuda.synchronize()
        counts = {"matched": int(((det_flags == 0) & (assign >= 0)).sum()), "spawned": int(spawned.sum()),
                  "retired": int((work[1] == _lib.TRACK_FLAG_RETIRED).sum())}
        v = sorted(event_time(launch, iters, 2) for _ in range(5))
        r = sorted(event_time(restore, 50, 2) for _ in range(5))
        return v[2], v[4] - v[0], r[2], counts

    free = np.where(np.arange(len(flat)) % 4 == 3, _lib.TRACK_FLAG_PREVIOUS, 0).astype(np.int32)
    moved = flat + rng.integers(-6, 7, flat.shape).astype(np.int32) * np.array([1, 1, 0, 0], np.int32)
    many = np.concatenate([rng.integers(0, W - 60, (CAP, 1)), rng.integers(0, H - 60, (CAP, 1)), rng.integers(20, 61, (CAP, 2))], axis=1)
    many_frames = rng.integers(0, FRAMES, CAP)
    found = many + rng.integers(-8, 9, many.shape) * np.array([1, 1, 0, 0])
    order = rng.permutation(CAP)
    same = np.tile(np.array([[100, 100, 200, 200]]), (CAP, 1))
    nested = np.stack([np.full(CAP, 100), np.full(CAP, 100), 2000 + 1 + np.arange(CAP), np.full(CAP, 2000)], axis=1)
    inner = np.tile(np.array([[100, 100, 2000, 2000]]), (CAP, 1))
    zeros = np.zeros(CAP, np.int32)
    for name, args in (("assign_64", (np.where(free[:, None] != 0, 0, flat), free, index, moved, index, FRAMES, 200)),
                       ("assign_cap_random", (many, zeros, many_frames, found[order], many_frames[order], FRAMES, 50)),
                       ("assign_cap_identical", (same, zeros, zeros, same, zeros, 1, 10)),
                       ("assign_cap_nested", (nested, zeros, zeros, inner, zeros, 1, 3))):
        res[name + "_s"], res[name + "_spread_s"], res["restore_" + name[7:] + "_s"], res[name + "_counts"] = case(*args)

    # ---- the loop ----
    trackers = {k: HeadTracker(pred) for k in ("step_only_loop_s", "spare_loop_s", "device_loop_s", "host_loop_s")}
    log = []

    def loop(mode):
        tracker = trackers[mode]
        tracker.start(d_frames, d_start, d_index, n_slots=None if mode == "step_only_loop_s" else SLOTS)
        misses = np.zeros(SLOTS, np.int32)
        log.clear()
        for _ in range(steps):
            tracker.step(d_frames)
            if mode == "device_loop_s":
                a = tracker.update(d_start, d_index, d_count, match_iou=MATCH_IOU, max_misses=MAX_MISSES)
                log.append(a.spawned)
            elif mode == "host_loop_s":
                lost, held = tracker.lost().cpu().numpy(), tracker.boxes().cpu().numpy()  # the host wait
                a = host_boxes.assign_detections(held, lost, tracker._index.cpu().numpy(), misses, flat, index, FRAMES, MATCH_IOU, max_misses=MAX_MISSES)
                misses = a.misses
                fresh = np.flatnonzero(a.spawned)
                if len(fresh):  # reseed cannot move a slot to another frame nor retire one: the host loop does less than update
                    tracker.reseed(fresh, a.boxes[fresh])
                log.append(a.spawned)
        torch.cuda.synchronize()

    for mode in trackers:  # warm-up: MIOpen picks its kernels for the batch
        loop(mode)
    times = {k: [] for k in trackers}
    spawned = {}
    for _ in range(5):
        for mode in trackers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(mode)
            times[mode].append(time.perf_counter() - t0)
            spawned[mode] = [int(np.asarray(s.cpu() if torch.is_tensor(s) else s).sum()) for s in log]
    for k, v in times.items():
        v.sort()
        res[k], res[k[:-2] + "_spread_s"] = v[2], v[4] - v[0]
        res[k[:-7] + "_per_step_s"] = v[2] / steps
    res["spawned_per_step"] = {k: v for k, v in spawned.items() if v}
    res["device_minus_spare_per_step_s"] = res["device_per_step_s"] - res["spare_per_step_s"]
    res["host_minus_spare_per_step_s"] = res["host_per_step_s"] - res["spare_per_step_s"]
    res["clock_mhz"].append(clock_mhz())
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
