#!/usr/bin/env python3
"""The occlusion-aware texture bake (csrc/uv_texture_occlusion.hip) on one MI355X: what the depth test costs, and how much it hides. Not
collected by pytest.

The set-up of bench_texture_frames.py: 8 frames of 1080 x 1920 on the device with 8 heads each, heads of 120 .. 500 pixels, some over the
frame's edges; the synthetic FLAME model's decoded vertices, the synthetic 256 x 256 atlas; depth maps of 512 x 512 per head.
  depth_frames_s                     `UVMap.depth_frames` alone: window, clear and raster launches for all 64 heads
  accumulate_launch_s                `UVMap.bake_frames` with a score (the launch of `TextureAccumulator.add`), without the depth test
  accumulate_occluded_launch_s       `dad3d_uvmap_bake_frames_occluded` alone, with a score, on depth maps drawn before
  add_s / add_occluded_s             `TextureAccumulator.add` on [64,413] params without and with `occlusion="self"`
  hidden_share                       of the candidates that pass the reference's two tests, the share the depth test hides, with the default
                                     biases 1.0 and 1.0 (counted with torch in float64 on the device's own depth maps and normals)
CUDA-event times around `iters` calls, the median of five such loops, the legs alternating; `*_spread_s` is the largest minus the
smallest of the five. The numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_texture_occlusion.py [--out profiles/texture_occlusion_bench.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, synthetic  # noqa: E402
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames  # noqa: E402
from dad_3dheads_amd.uv_texture import TextureAccumulator, UVTextureCreator  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W, S, D = 8, 8, 1080, 1920, 256, 512


def hidden_share(atlas, verts, normals, depth, window, flags, depth_bias=1.0, slope_bias=1.0):
    """(accepted, hidden) over the unflagged heads: the three tests in float64, every product and sum an operation of its own."""
    vf = torch.from_numpy(np.asarray(atlas["valid_pixel_3d_faces"], np.int64)).cuda()
    bc = torch.from_numpy(np.asarray(atlas["valid_pixel_b_coords"], np.float64)).cuda()
    accepted = hidden = 0
    for k in range(verts.shape[0]):
        if int(flags[k]):
            continue
        v, n = verts[k].double(), normals[k]
        p = (v[vf[:, 0]] * bc[:, 0:1] + v[vf[:, 1]] * bc[:, 1:2]) + v[vf[:, 2]] * bc[:, 2:3]
        pn = (n[vf[:, 0]] * bc[:, 0:1] + n[vf[:, 1]] * bc[:, 1:2]) + n[vf[:, 2]] * bc[:, 2:3]
        ndv = -pn[:, 2]
        rx, ry = torch.round(p[:, 0]), torch.round(p[:, 1])
        ok = ~(ndv < 0) & (rx > 0) & (rx < W) & (ry > 0) & (ry < H)
        x0, y0, ww, wh = window[k].tolist()
        ix, iy = rx.long() - x0, ry.long() - y0
        inside = ok & (ix >= 0) & (ix < ww) & (iy >= 0) & (iy < wh)
        d = torch.full_like(ndv, float("inf"))
        d[inside] = depth[k][iy[inside], ix[inside]].double()
        hid = ok & (p[:, 2] > d + (depth_bias + slope_bias * ((pn[:, 0].abs() + pn[:, 1].abs()) / ndv)))
        accepted += int(ok.sum())
        hidden += int(hid.sum())
    return accepted, hidden


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 10
    _lib.require_gpu()
    torch.cuda.set_device(0)
    lib = _lib.load()
    static = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, static)
    atlas = dict(synthetic.synthetic_texture_data(S, seed=0, static=static))
    creator = UVTextureCreator(texture_data=atlas, flame_model=model, static=static, device=0)
    flame = creator.head_mesh.flame
    n = FRAMES * PER_FRAME
    params = torch.from_numpy(synthetic.synthetic_params(n, seed=3)).cuda()
    raw = flame.decode(params.clone(), proj=True, to_2d=False)["proj"].cpu().numpy()
    rng = np.random.default_rng(0)
    verts = np.empty_like(raw)
    for k in range(n):  # heads of 120 .. 500 pixels, some over the frame's edges
        size = rng.integers(120, 500)
        cx, cy = rng.integers(-40, W - 100) + size / 2, rng.integers(-40, H - 100) + size / 2
        lo, hi = raw[k, :, :2].min(0), raw[k, :, :2].max(0)
        s = np.float32(size / (hi - lo).max())
        verts[k] = (raw[k] - np.float32([*(lo + hi) / 2, 0.0])) * s + np.float32([cx, cy, 0.0])
    v_bake = torch.from_numpy(verts).cuda()
    d_index = torch.arange(FRAMES, dtype=torch.int32).repeat_interleave(PER_FRAME).cuda()
    frames = torch.from_numpy(rng.integers(0, 256, (FRAMES, H, W, 3), dtype=np.uint8)).cuda()
    table = DeviceFrames(frames, torch.device("cuda", 0))
    res = {"device": torch.cuda.get_device_name(0), "build": lib.dad3d_build_info().decode(), "frames": [FRAMES, H, W], "heads": n,
           "texture_size": S, "depth_side": D, "depth_bias": 1.0, "slope_bias": 1.0, "iters": iters}

    def medians(legs):
        times = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                times[k].append(event_time(fn, iters, 2))
        for k, t in times.items():
            t.sort()
            res[f"{k}_s"], res[f"{k}_spread_s"] = t[2], t[4] - t[0]

    m = creator.uv_map
    normals = m.vertex_normals(v_bake)
    maps = m.depth_frames(v_bake, table, d_index, depth_side=D)
    depth, window, d_flags = maps
    plain = TextureAccumulator(creator, n)
    occluded = TextureAccumulator(creator, n, occlusion="self", depth_side=D)
    flags = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def occluded_launch():
        _lib.check(lib.dad3d_uvmap_bake_frames_occluded(
            m._handle, occluded.textures.data_ptr(), occluded.score.data_ptr(), v_bake.data_ptr(), normals.data_ptr(), table.device.data_ptr(),
            table.host.ctypes.data, len(table), d_index.data_ptr(), n, depth.data_ptr(), window.data_ptr(), d_flags.data_ptr(), D,
            C.c_double(1.0), C.c_double(1.0), flags.data_ptr(), stream))

    occluded_launch()
    torch.cuda.synchronize()
    res["depth_flags_set"] = int((d_flags != 0).sum())
    res["window_pixels"] = int((window[:, 2].long() * window[:, 3].long()).sum())
    res["covered_pixels"] = int(sum(int(torch.isfinite(depth[k, :int(window[k, 3]), :int(window[k, 2])]).sum()) for k in range(n)))
    accepted, hidden = hidden_share(atlas, v_bake, normals, depth, window, d_flags)
    res["accepted_candidates"], res["hidden_candidates"], res["hidden_share"] = accepted, hidden, hidden / max(accepted, 1)
    a0, h0 = hidden_share(atlas, v_bake, normals, depth, window, d_flags, 0.0, 0.0)
    res["hidden_share_without_biases"] = h0 / max(a0, 1)
    medians({"depth_frames": lambda: m.depth_frames(v_bake, table, d_index, depth_side=D, out=maps),
             "accumulate_launch": lambda: m.bake_frames(v_bake, normals, table, d_index, out=plain.textures, score=plain.score),
             "accumulate_occluded_launch": occluded_launch,
             "add": lambda: plain.add(params, table, d_index),
             "add_occluded": lambda: occluded.add(params, table, d_index)})
    res["texels_filled"], res["texels_filled_occluded"] = int(plain.filled().sum()), int(occluded.filled().sum())
    res["texels_differing"] = int((plain.textures != occluded.textures).any(-1).sum())
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
