#!/usr/bin/env python3
"""Time of the textured head render (`Mesh.render_texture`, `UVTextureCreator.render_batch`; csrc/sim3dr_kernels.hip
`render_texture_kernel`) on one MI355X, beside the per-vertex-colour raster of the same vertices. Not collected by pytest.

Inputs: seeded synthetic params ("crop" profile: the head fills the 256 x 256 frame), the synthetic atlas' corner layout
(`synthetic.synthetic_texcoords`), random 256 x 256 x 3 uint8 textures, one per head. Per batch size B (64 and 256), in ONE process:
  textured_nearest_s / textured_bilinear_s   geometry + tile launches of `Mesh.render_texture` on decoded vertices (uint8 image)
  render_batch_s                             `render_batch` end to end: fused decode + the two launches
  vertex_colour_s                            `Mesh.rasterize` on the same vertices and the same triangle list with per-vertex colours:
                                             the yardstick -- the same geometry launch and the same coverage work without the
                                             texel gathers, through the tuned tile kernel
  ratio_textured_over_vertex_colour          textured_bilinear_s / vertex_colour_s
and, when oracle/_ref holds the compiled reference, `_render_texture_core` on one core (seconds per head).
Every batch size runs as a child process under its own time limit; after a failed step nothing more is started.

    python tests/perf/bench_render_texture.py [--out profiles/render_texture_bench.json]
"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

BATCHES = (64, 256)
STEP_LIMIT_S = 240
H = W = S = 256


def step(b, iters=50):
    import numpy as np
    import torch

    import render_texture_ref as RT
    from dad_3dheads_amd import _lib, synthetic
    from dad_3dheads_amd.Sim3DR import Mesh
    from dad_3dheads_amd.uv_texture import UVTextureCreator, texel_coords
    from event_timer import event_time

    _lib.require_gpu()
    torch.cuda.set_device(0)
    static = synthetic.load_static()
    atlas = dict(synthetic.synthetic_texture_data(S, seed=0, static=static))
    atlas.update(synthetic.synthetic_texcoords(S, static))
    creator = UVTextureCreator(texture_data=atlas, flame_model=synthetic.synthetic_flame_model(0, static), static=static, device=0)
    mesh = creator.renderer
    rng = np.random.default_rng(b)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=b)).cuda()
    textures = torch.from_numpy(rng.integers(0, 256, (b, S, S, 3), dtype=np.uint8)).cuda()
    verts = creator.head_mesh.flame.decode(params, proj=True, to_2d=False, flip_z=True, mutate=True)["proj"]
    img = torch.zeros((b, H, W, 3), dtype=torch.uint8, device="cuda")
    creator.reserve_render(b, (H, W))
    # the yardstick: the same triangles (the faces that have texture coordinates) with per-vertex colours
    kept = (atlas["ft"] >= 0).all(1)
    plain = Mesh(np.ascontiguousarray(static["faces"][kept], dtype=np.int32), mesh.nver, device=0)
    colors = torch.from_numpy(rng.uniform(0, 1, (b, mesh.nver, 3)).astype(np.float32)).cuda()
    res = {"B": b, "image": [H, W, 3], "texture": [S, S, 3], "triangles": mesh.ntri}
    res["vertex_colour_s"] = event_time(lambda: plain.rasterize(verts, colors, img), iters, 3)
    res["textured_nearest_s"] = event_time(lambda: mesh.render_texture(verts, textures, img, mapping="nearest"), iters, 3)
    res["textured_bilinear_s"] = event_time(lambda: mesh.render_texture(verts, textures, img, mapping="bilinear"), iters, 3)
    res["render_batch_s"] = event_time(lambda: creator.render_batch(params, textures, out=img), iters, 3)
    res["vertex_colour_again_s"] = event_time(lambda: plain.rasterize(verts, colors, img), iters, 3)  # drift of the yardstick
    res["ratio_textured_over_vertex_colour"] = res["textured_bilinear_s"] / res["vertex_colour_s"]
    res["heads_per_s_textured_bilinear"] = b / res["textured_bilinear_s"]
    res["pixels_drawn_per_head"] = float((img.reshape(b, -1, 3).amax(-1) > 0).sum().item()) / b
    if b == BATCHES[0] and RT.ref_available():  # the compiled reference on one core, three heads
        v = verts[:3].cpu().numpy()
        tc2 = texel_coords(atlas["vt"], S).astype(np.float32)
        faces_kept, ft = np.ascontiguousarray(static["faces"][kept], dtype=np.int32), np.ascontiguousarray(atlas["ft"][kept], dtype=np.int32)
        tex = textures[0].cpu().numpy().astype(np.float32)
        cases = [RT.unrolled(v[i], faces_kept, tc2, ft) for i in range(len(v))]
        t0 = time.perf_counter()
        for uv, ut, utc, utt in cases:
            RT.ref_render(uv, ut, tex, utc, utt, H, W, 3, 1)
        res["reference_one_core_s_per_head"] = (time.perf_counter() - t0) / len(cases)
    res["device"] = torch.cuda.get_device_name(0)
    res["build"] = _lib.load().dad3d_build_info().decode()
    print("STEP " + json.dumps(res), flush=True)


def main():
    argv = sys.argv[1:]
    if "--step" in argv:
        return step(int(argv[argv.index("--step") + 1]))
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    steps = []
    for b in BATCHES:
        try:
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(b)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"step B={b}: no result within {STEP_LIMIT_S} s; nothing more is started", file=sys.stderr)
            return 1
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("STEP ")]
        if proc.returncode != 0 or not lines:
            sys.stderr.write(proc.stdout[-2000:] + proc.stderr[-4000:])
            print(f"step B={b} failed with status {proc.returncode}; nothing more is started", file=sys.stderr)
            return 1
        steps.append(json.loads(lines[-1][5:]))
    res = {"device": steps[0].pop("device"), "build": steps[0].pop("build"), "steps": steps}
    for s in steps[1:]:
        s.pop("device"), s.pop("build")
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
