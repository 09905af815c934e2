#!/usr/bin/env python3
"""The overlays (dad-3dheads_amd/overlay.py, csrc/overlay.hip) on one MI355X beside PIL's `ImageDraw.line` over the same segments on
the host, in the same process. Not collected by pytest.

The vertices are the fused decode's projection of synthetic parameters, scaled to the image; the edge list is the first 10 938
(the length of the reference's head_edges.npy) of `overlay.mesh_edges()`. Two shapes: B = 64 of 256 x 256 and B = 8 of 954 x 766.
  draw_mesh_s           `overlay.draw_mesh` with the edge list on the device: one launch (CUDA events, after warm-up)
  draw_mesh_in_place_s  the same with `out=` the images
  draw_3d_landmarks_s   `overlay.draw_3d_landmarks(.., "445")`
  segments_kernel_s / discs_kernel_s   the two C-ABI calls alone, in place (no allocation)
  pil_lines_s           `ImageDraw.line` per segment on the copied-back vertices, every image of the batch (host clock, one run)
PIL draws other pixels (its own line rule, no anti-aliasing): it is a yardstick for time only. The numbers are recorded as
measured; no condition is asserted on them.

    python tests/perf/bench_overlay.py [--out profiles/overlay_bench.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, landmarks, overlay, synthetic  # noqa: E402
from dad_3dheads_amd.head_mesh import HeadMesh  # noqa: E402
from event_timer import event_time  # noqa: E402

N_EDGES = 10938


def projected(batch, h, w):
    static = synthetic.load_static()
    hm = HeadMesh(flame_model=synthetic.synthetic_flame_model(0, static), landmarks=landmarks.canonical("445", static), static=static, device=0)
    params = torch.from_numpy(synthetic.synthetic_params(batch, seed=21)).cuda()
    proj = hm.decode(params, to_2d=True, landmarks=False)["proj"]  # pixels of a 256 x 256 crop
    return (proj[..., :2] * torch.tensor([w / 256.0, h / 256.0], device="cuda")).contiguous()


def pil_lines(images, verts, edges):
    out = []
    for img, v in zip(images, verts.astype(int)):
        pil = Image.fromarray(img)
        draw = ImageDraw.Draw(pil)
        for a, b in edges:
            draw.line([tuple(v[a]), tuple(v[b])], fill=overlay.EDGE_COLOR, width=1)
        out.append(pil)
    return out


def measure(batch, h, w, iters):
    verts = projected(batch, h, w)
    torch.manual_seed(batch)
    images = torch.randint(0, 256, (batch, h, w, 3), dtype=torch.uint8, device="cuda")
    edges_host = overlay.mesh_edges()[:N_EDGES]
    edges = torch.from_numpy(edges_host).cuda()
    pred = {"projected_vertices": verts}
    work = images.clone()
    inside = ((verts[..., 0] >= 0) & (verts[..., 0] < w) & (verts[..., 1] >= 0) & (verts[..., 1] < h)).float().mean().item()
    ids = torch.from_numpy(overlay.landmark_indices("445").copy()).cuda()
    rgb, radius = overlay._color(overlay.EDGE_COLOR), overlay.default_radius(h, w)
    res = {"B": batch, "shape": [h, w, 3], "edges": int(edges.shape[0]), "vertices_inside_image": inside,
           "draw_mesh_s": event_time(lambda: overlay.draw_mesh(pred, images, edges), iters, 3),
           "draw_mesh_in_place_s": event_time(lambda: overlay.draw_mesh(pred, work, edges, out=work), iters, 3),
           "draw_3d_landmarks_s": event_time(lambda: overlay.draw_3d_landmarks(pred, images, "445"), iters, 3),
           "segments_kernel_s": event_time(lambda: overlay._launch_segments(work, work, verts, edges, None, rgb, 0), iters, 3),
           "discs_kernel_s": event_time(lambda: overlay._launch_discs(work, work, verts, ids, radius, rgb), iters, 3)}
    drawn = overlay.draw_mesh(pred, images, edges)
    res["pixels_changed_per_image"] = int((drawn != images).any(3).sum().item() // batch)
    host_images, host_verts = images.cpu().numpy(), verts.cpu().numpy()
    t0 = time.perf_counter()
    pil_lines(host_images, host_verts, edges_host)
    res["pil_lines_s"] = time.perf_counter() - t0
    res["speedup_vs_pil_lines"] = res["pil_lines_s"] / res["draw_mesh_s"]
    return res


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
           "runs": [measure(64, 256, 256, iters=20), measure(8, 954, 766, iters=20)]}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
