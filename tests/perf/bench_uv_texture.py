#!/usr/bin/env python3
"""Throughput of the UV-texture bake (dad-3dheads_amd/uv_texture.py, csrc/uv_texture.hip) on one MI355X, beside the float64 CPU
restatement of tests/uv_texture_restatement.py. Not collected by pytest.

Inputs: the synthetic atlas (`synthetic.synthetic_texture_data(S)`), seeded synthetic params, random 256 x 256 photos. Per (B, S):
  kernels_s            the two kernels alone (float64 normals + texel bake) on decoded vertices, CUDA events
  bake_batch_s         `bake_batch` end to end (fused decode + normals + bake) on device tensors
  textures_per_s_*     B / the matching time
  roofline             bytes the two kernels must move at least: texture writes + photo pixels gathered (one 3-byte pixel per
                       candidate, an upper bound) + the candidate table once per chunk of 8 images + vertices and normals
                       (fp32 positions read, float64 normals written and read); `bound_s` = bytes / 8 TB/s
The CPU restatement is timed per texture (S = 256).

    python tests/perf/bench_uv_texture.py [--out profiles/uv_texture_bench.json]
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
sys.path.insert(0, os.path.dirname(HERE))
import uv_texture_restatement as R  # noqa: E402
from dad_3dheads_amd import _lib, synthetic  # noqa: E402
from dad_3dheads_amd.uv_texture import UVTextureCreator  # noqa: E402
from event_timer import event_time  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
CHUNK = 8  # kUvBakeChunk


def run(creator, td, b, iters):
    m = creator.uv_map
    s, n_cand, v = m.size, len(td["valid_pixel_ids"]), m.n_verts
    rng = np.random.default_rng(b)
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=b)).cuda()
    images = torch.from_numpy(rng.integers(0, 256, (b, 256, 256, 3), dtype=np.uint8)).cuda()
    verts = creator.head_mesh.flame.decode(params.clone(), proj=True, to_2d=False, mutate=True)["proj"]
    normals = torch.empty((b, v, 3), dtype=torch.float64, device="cuda")
    tex = torch.empty((b, s, s, 3), dtype=torch.uint8, device="cuda")
    creator.reserve(b)

    def kernels():
        m.vertex_normals(verts, out=normals)
        m.bake(verts, normals, images, out=tex)

    t_k = event_time(kernels, iters, 1)
    t_b = event_time(lambda: creator.bake_batch(params, images, out=tex), iters, 1)
    n_norm = event_time(lambda: m.vertex_normals(verts, out=normals), iters, 1)
    written = int(tex.any(-1).sum().item())
    chunks = (b + CHUNK - 1) // CHUNK
    nbytes = {"texture_writes": b * s * s * 3, "photo_gathers": b * n_cand * 3,
              "table_per_chunk": chunks * (n_cand * (12 + 24) + (s * s + 1) * 4),
              "vertices_normals": b * v * (12 + 24 + 12 + 24)}  # normals kernel: read fp32, write f64; bake: read both
    total = sum(nbytes.values())
    return {"B": b, "S": s, "candidates": n_cand, "texels_written": written, "kernels_s": t_k, "normals_kernel_s": n_norm,
            "bake_batch_s": t_b, "textures_per_s_kernels": b / t_k, "textures_per_s_bake_batch": b / t_b,
            "roofline": {"bytes": nbytes, "total_bytes": total, "bound_s": total / HBM_BYTES_PER_S,
                         "fraction_of_bound": (total / HBM_BYTES_PER_S) / t_k}}


def cpu_restatement(td, faces, n):
    params = synthetic.synthetic_params(n, seed=5)
    from oracle import flame_ref

    consts = flame_ref.FlameConstants.from_model(synthetic.synthetic_flame_model(0))
    verts = flame_ref.reprojected_vertices(consts, torch.from_numpy(params), to_2d=False).numpy()
    img = np.random.default_rng(0).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    for i in range(n):
        R.compute_texture_map(td, img, verts[i], faces)
    dt = time.perf_counter() - t0
    return {"textures": n, "S": int(td["img_size"]), "seconds_per_texture": dt / n}


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    _lib.require_gpu()
    torch.cuda.set_device(0)
    static = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, static)
    gpu = []
    atlas256 = None
    for s in (256, 512):
        td = synthetic.synthetic_texture_data(s, seed=0, static=static)
        atlas256 = td if s == 256 else atlas256
        creator = UVTextureCreator(texture_data=td, flame_model=model, static=static, device=0)
        for b in (1, 16, 64):
            gpu.append(run(creator, td, b, iters=50))
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "gpu": gpu,
           "cpu_float64_restatement": cpu_restatement(atlas256, static["faces"], 3)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
