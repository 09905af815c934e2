#!/usr/bin/env python3
"""The textures of tracked heads (csrc/uv_texture_frames.hip, csrc/sim3dr_frames_texture.hip) on one MI355X, each beside the route that
existed before it, in the same process. Not collected by pytest.

The set-up of bench_render_frames.py: 8 frames of 1080 x 1920 on the device with 8 heads each, heads of 120 .. 500 pixels, some over
the frame's edges; the synthetic FLAME model's decoded vertices, the synthetic 256 x 256 atlas and its corner layout.
  bake_gather_s / bake_frames_s     the plain bake of all 64 heads: gather `frames[image_index]` into a [64,H,W,3] batch (398 MB) and
                                    `UVMap.bake`, against one `UVMap.bake_frames` on the 8 frames (vertices and normals given to both)
  accumulate_launch_s               `UVMap.bake_frames` with a score: the launch of `TextureAccumulator.add` alone
  accumulate_add_s                  `TextureAccumulator.add` on [64,413] params: decode, float64 normals and that launch
  render_per_head_s / render_frames_s   64 calls of `Mesh.render_texture` with a batch of one on a [1,H,W,3] view of the head's frame,
                                    in order, against one `Mesh.render_texture_frames`; bilinear, uint8 textures [64,256,256,3]
The bytes of the two routes are compared once, on fresh frames, before anything is timed (`*_bytes_equal`). CUDA-event times around
`iters` calls, the median of five such loops, the routes alternating; `*_spread_s` is the largest minus the smallest of the five. The
numbers are recorded as measured; no condition is asserted on them.

    python tests/perf/bench_texture_frames.py [--out profiles/texture_frames_bench.json]
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
from dad_3dheads_amd.Sim3DR.frames import DeviceFrames  # noqa: E402
from dad_3dheads_amd.uv_texture import TextureAccumulator, UVTextureCreator  # noqa: E402
from event_timer import event_time  # noqa: E402

FRAMES, PER_FRAME, H, W, S = 8, 8, 1080, 1920, 256


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 10
    _lib.require_gpu()
    torch.cuda.set_device(0)
    static = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, static)
    atlas = dict(synthetic.synthetic_texture_data(S, seed=0, static=static))
    atlas.update(synthetic.synthetic_texcoords(S, static))
    creator = UVTextureCreator(texture_data=atlas, flame_model=model, static=static, device=0)
    flame = creator.head_mesh.flame
    n = FRAMES * PER_FRAME
    params = torch.from_numpy(synthetic.synthetic_params(n, seed=3)).cuda()
    raw = {flip: flame.decode(params.clone(), proj=True, to_2d=False, flip_z=flip)["proj"].cpu().numpy() for flip in (False, True)}
    rng = np.random.default_rng(0)
    verts = {flip: np.empty_like(raw[flip]) for flip in raw}
    for k in range(n):  # heads of 120 .. 500 pixels, some over the frame's edges
        size = rng.integers(120, 500)
        cx, cy = rng.integers(-40, W - 100) + size / 2, rng.integers(-40, H - 100) + size / 2
        lo, hi = raw[True][k, :, :2].min(0), raw[True][k, :, :2].max(0)
        s = np.float32(size / (hi - lo).max())
        for flip in raw:
            verts[flip][k] = (raw[flip][k] - np.float32([*(lo + hi) / 2, 0.0])) * s + np.float32([cx, cy, 0.0])
    v_bake, v_draw = torch.from_numpy(verts[False]).cuda(), torch.from_numpy(verts[True]).cuda()
    index = torch.arange(FRAMES, dtype=torch.int32).repeat_interleave(PER_FRAME)
    d_index, d_long = index.cuda(), index.cuda().long()
    bg = torch.from_numpy(rng.integers(0, 256, (FRAMES, H, W, 3), dtype=np.uint8)).cuda()
    work = bg.clone()
    table = DeviceFrames(work, torch.device("cuda", 0))
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "frames": [FRAMES, H, W], "heads": n,
           "texture_size": S, "iters": iters}

    def medians(name, legs):
        times = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                times[k].append(event_time(fn, iters, 2))
        for k, t in times.items():
            t.sort()
            res[f"{name}_{k}_s"], res[f"{name}_{k}_spread_s"] = t[2], t[4] - t[0]

    # ---- the plain bake -----------------------------------------------------------------------------------------------------
    m = creator.uv_map
    normals = m.vertex_normals(v_bake)
    tex_a = torch.empty((n, S, S, 3), dtype=torch.uint8, device="cuda")
    tex_b = torch.empty_like(tex_a)

    def gather_route():
        m.bake(v_bake, normals, work.index_select(0, d_long), out=tex_a)

    def frames_route():
        m.bake_frames(v_bake, normals, table, d_index, out=tex_b)

    gather_route()
    _, flags = m.bake_frames(v_bake, normals, table, d_index, out=tex_b)
    torch.cuda.synchronize()
    res["bake_bytes_equal"] = bool(torch.equal(tex_a, tex_b))
    res["bake_flags_set"] = int((flags != 0).sum())
    res["bake_texels_filled"] = int(tex_b.any(-1).sum())
    res["bake_gathered_bytes"] = int(n * H * W * 3)
    medians("bake", {"gather": gather_route, "frames": frames_route})
    res["bake_speedup"] = res["bake_gather_s"] / res["bake_frames_s"]

    # ---- accumulation -------------------------------------------------------------------------------------------------------
    acc = TextureAccumulator(creator, n)
    medians("accumulate", {"launch": lambda: m.bake_frames(v_bake, normals, table, d_index, out=acc.textures, score=acc.score),
                           "add": lambda: acc.add(params, table, d_index)})
    res["accumulate_texels_filled"] = int(acc.filled().sum())

    # ---- the textured render ------------------------------------------------------------------------------------------------
    mesh = creator.renderer
    textures = tex_b

    def per_head(frames):
        for k in range(n):
            mesh.render_texture(v_draw[k:k + 1], textures[k], frames[int(index[k])][None])

    a = bg.clone()
    per_head(a)
    work.copy_(bg)
    flags = mesh.render_texture_frames(table, v_draw, textures, d_index)
    torch.cuda.synchronize()
    res["render_bytes_equal"] = bool(torch.equal(a, work))
    res["render_flags_set"] = int((flags != 0).sum())
    res["render_pixels_drawn"] = int((work != bg).any(3).sum())
    medians("render", {"per_head": lambda: per_head(work), "frames": lambda: mesh.render_texture_frames(table, v_draw, textures, d_index)})
    res["render_speedup"] = res["render_per_head_s"] / res["render_frames_s"]
    res["frames_scratch_bytes"] = mesh.frames_scratch_bytes()
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
