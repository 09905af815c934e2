#!/usr/bin/env python3
"""`Mesh.render_frames` / `Mesh.rasterize_frames` (csrc/sim3dr_frames.hip) on one MI355X beside the route the batched entries offer for
several heads of a frame, in the same process: `Mesh.render(v[k:k+1], frame[None])` / `Mesh.rasterize(..)` once per head, in order.
Not collected by pytest.

The workload of bench_predict_boxes.py: 8 frames of 1080 x 1920 with 8 heads each, heads of 120 .. 500 pixels, some over the frame's
edges; the synthetic FLAME model's decoded vertices. `render_*`: the whole FLAME mesh under the default light; `pncc_*`: the ear-less
face subset with the NCC colour codes.
  *_per_head_s   64 calls of the batched entry with a batch of one on the head's whole frame (510 tiles a launch)
  *_frames_s     one call of the frames chain for all 64 heads
Both routes draw over what the call before left (the same work every time); the bytes of the two routes are compared once, on fresh
frames, before anything is timed (`*_bytes_equal`). CUDA-event times around `iters` calls, the median of five such loops, the routes
alternating; `*_spread_s` is the largest minus the smallest of the five. The numbers are recorded as measured; no condition is
asserted on them.

    python tests/perf/bench_render_frames.py [--out profiles/render_frames_bench.json]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, synthetic  # noqa: E402
from dad_3dheads_amd.head_mesh import HeadMesh  # noqa: E402
from dad_3dheads_amd.pncc import compute_ncc_color_codes  # noqa: E402
from dad_3dheads_amd.Sim3DR import Mesh  # noqa: E402
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W = 8, 8, 1080, 1920


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 10
    _lib.require_gpu()
    torch.cuda.set_device(0)
    static = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, static)
    hm = HeadMesh(flame_model=model, static=static, device=0)
    n = FRAMES * PER_FRAME
    params = torch.from_numpy(synthetic.synthetic_params(n, seed=3)).cuda()
    raw = hm.flame.decode(params, proj=True, to_2d=False, flip_z=True)["proj"].cpu().numpy()
    rng = np.random.default_rng(0)
    verts = np.empty_like(raw)
    for k in range(n):  # heads of 120 .. 500 pixels, some over the frame's edges
        size = rng.integers(120, 500)
        cx, cy = rng.integers(-40, W - 100) + size / 2, rng.integers(-40, H - 100) + size / 2
        lo, hi = raw[k, :, :2].min(0), raw[k, :, :2].max(0)
        s = np.float32(size / (hi - lo).max())
        verts[k] = (raw[k] - np.float32([*(lo + hi) / 2, 0.0])) * s + np.float32([cx, cy, 0.0])
    v = torch.from_numpy(verts).cuda()
    index = torch.arange(FRAMES, dtype=torch.int32).repeat_interleave(PER_FRAME)
    d_index = index.cuda()
    bg = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(FRAMES)]

    faces = np.ascontiguousarray(static["faces"], dtype=np.int32)
    faces_pncc = np.ascontiguousarray(static["faces_wo_ears"], dtype=np.int32)
    nver = verts.shape[1]
    full, face = Mesh(faces, nver, device=0), Mesh(faces_pncc, nver, device=0)
    ncc = compute_ncc_color_codes(np.asarray(model.v_template), np.unique(faces_pncc)).astype(np.float32)
    col = torch.from_numpy(ncc).cuda()[None].expand(n, -1, -1).contiguous()

    def per_head(draw, frames):
        for k in range(n):
            draw(k, frames[int(index[k])][None])

    routes = {
        "render": (lambda frames: per_head(lambda k, f: full.render(v[k:k + 1], f), frames),
                   lambda frames, table: full.render_frames(table, v, d_index)),
        "pncc": (lambda frames: per_head(lambda k, f: face.rasterize(v[k:k + 1], col[k:k + 1], f), frames),
                 lambda frames, table: face.rasterize_frames(table, v, col, d_index)),
    }
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W], "heads": n,
           "iters": iters}
    work = [b.clone() for b in bg]
    table = DeviceFrames(work, torch.device("cuda", 0))
    for name, (old, new) in routes.items():
        a = [b.clone() for b in bg]
        old(a)
        for w, b in zip(work, bg):
            w.copy_(b)
        flags = new(work, table)
        torch.cuda.synchronize()
        res[f"{name}_bytes_equal"] = bool(all(torch.equal(x, y) for x, y in zip(a, work)))
        res[f"{name}_flags_set"] = int((flags != 0).sum())
        res[f"{name}_pixels_drawn"] = int(sum((x != b).any(2).sum() for x, b in zip(work, bg)))
        times = {"per_head": [], "frames": []}
        for _ in range(5):
            times["per_head"].append(event_time(lambda: old(work), iters, 2))
            times["frames"].append(event_time(lambda: new(work, table), iters, 2))
        for k, t in times.items():
            t.sort()
            res[f"{name}_{k}_s"], res[f"{name}_{k}_spread_s"] = t[2], t[4] - t[0]
        res[f"{name}_speedup"] = res[f"{name}_per_head_s"] / res[f"{name}_frames_s"]
    res["frames_scratch_bytes"] = [full.frames_scratch_bytes(), face.frames_scratch_bytes()]
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
