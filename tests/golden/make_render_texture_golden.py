#!/usr/bin/env python3
"""Generate tests/golden/render_texture_golden.npz from the reference's own `_render_texture_core`
(Sim3DR/lib/rasterize_kernel.cpp:358-463).

Authoring-container only: needs oracle/_ref/libsim3dr_ref.so (oracle/Makefile). Cases, all 96x96 with a 64x64x3 float
texture and the real FLAME topology (faces from assets/flame_static.npz, not stored again), texture coordinates per vertex
(`tex_triangles == triangles`, so reference and corner indexing name the same texels):

  centre   the head in the middle of the frame: no pixel of the two-pixel border band is drawn
  left     the same head shifted so that it crosses the left edge: band pixels are drawn by every triangle whose box reaches
           them -- the case that pins the band rule of :423

each with mapping_type 0 (nearest) and 1 (bilinear): float image and depth buffer as the reference leaves them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_texture_ref as RT  # noqa: E402
from dad_3dheads_amd import synthetic  # noqa: E402

H = W = 96
S = 64


def main():
    st = synthetic.load_static()
    faces = np.ascontiguousarray(st["faces"], dtype=np.int32)
    tex = RT.smooth_texture(S, S, 3, seed=3)
    tc = RT.head_texcoords(st, S)
    band = RT.band_mask(H, W)
    out = {"texture": tex, "tex_coords": tc}
    band_drawn = 0
    for name, shift in (("centre", 0.0), ("left", -40.0)):
        v = RT.head_vertices(st, H, W, shift_x=shift)
        out[f"{name}_vertices"] = v
        for mapping in (0, 1):
            img, dep = RT.ref_render(v, faces, tex, tc, faces, H, W, 3, mapping)
            drawn = dep > -1e8
            print(f"{name} mapping {mapping}: drawn {drawn.mean():.3f}, band pixels drawn {int((drawn & band).sum())} of {int(band.sum())}")
            band_drawn += int((drawn & band).sum())
            out[f"{name}_image{mapping}"] = img
            out[f"{name}_depth{mapping}"] = dep
    assert band_drawn > 0, "no case draws a band pixel: the band rule would go unchecked"
    np.savez_compressed(RT.GOLDEN, **out)
    print("wrote", RT.GOLDEN, os.path.getsize(RT.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
