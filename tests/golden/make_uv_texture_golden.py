#!/usr/bin/env python3
"""Build tests/golden/uv_texture_golden.npz: inputs and outputs of the reference's OWN `UVTextureCreator._compute_texture_map`
(inference/uv_texture.py:21-46), executed unmodified from the reference checkout.

Runs ONLY where the reference checkout is present (DAD3D_REFERENCE_ROOT, default /root/reference). Stand-ins for what is not
there:
  psbody.mesh   `Mesh` = tests/uv_texture_restatement.py `RestatedMesh` (psbody-mesh's `v` float64, `f` uint32 and
                `estimate_vertex_normals`, restated from its published source: unpinned here)
  model_training.head_mesh   an empty module (`__init__`, which loads the absent texture_data.npy / generic_model.pkl and the
                FLAME model, is never run: the creator is made with object.__new__ and given its `texture_data`)

Items (the photo is tests/golden/demo_image.npz `resized`, 256 x 206):
  0, 1   synthetic atlas S = 256, seed 0; oracle-decoded `to_2d=False` vertices of synthetic params rows 0 and 1, moved 25 px
         left over the photo
  2      synthetic atlas S = 256, seed 1, 4000 duplicate candidates (last writer wins); params row 2
  3      atlas of item 0; params row 3 with z negated (the other side faces the viewer)
  adv    a hand-made 40-vertex mesh with its own faces and a hand-made S = 16 atlas, over the photo's top-left 20 x 24 crop:
         degenerate faces (normal 0, n_dot_view = -0.0), a face naming a vertex twice, an isolated vertex, points on exact
         half-integers of both parities, x = 0, W-1, W, y = 0, H-1, H, NaN and inf vertices, negative (wrapping) and
         fractional (truncated) texel coordinates
The decoded items use the packaged FLAME face list (assets/flame_static.npz `faces`) as `generic_model.pkl['f']`, an
assumption: that file is absent.

Stored: the vertices, the textures, the atlas recipes with the sha256 of each synthetic atlas (the tests regenerate them), the
adversarial mesh and atlas whole (small), and the photo crop's geometry. Everything is synthetic input and the reference
function's output; the photo is the reference's demo image (see demo_image.npz).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DAD3D_REFERENCE_ROOT", "/root/reference")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "uv_texture_golden.npz")
SHIFT_X = 25.0
ADV_H, ADV_W, ADV_S = 20, 24, 16


def adversarial():
    """The hand-made mesh, atlas and crop of item `adv` (deterministic)."""
    rng = np.random.default_rng(77)
    n = 40
    v = np.zeros((n, 3), np.float32)
    # 0..23: a grid of points on half-integers and on the bounds, z of both signs
    xs = [0.0, 0.5, 1.5, 2.5, 3.5, 11.5, 12.5, 22.5, 23.0, 23.5, 24.0, 24.5]
    for i in range(24):
        v[i] = [xs[i % 12], [0.5, 1.5, 18.5, 19.5][i // 6] if i < 24 else 0, rng.uniform(-5, 5)]
    v[24] = [10.5, 10.5, 0.0]  # 24..26: a degenerate face (three equal points)
    v[25] = [10.5, 10.5, 0.0]
    v[26] = [10.5, 10.5, 0.0]
    v[27] = [7.0, 5.0, 2.0]    # 27..29: collinear
    v[28] = [8.0, 6.0, 3.0]
    v[29] = [9.0, 7.0, 4.0]
    v[30] = [np.nan, 3.0, 1.0]
    v[31] = [5.0, np.inf, 1.0]
    v[32] = [-np.inf, 4.0, 0.0]
    v[33] = [6.5, 20.0, -1.0]  # y = H
    v[34] = [4.5, 19.0, 1.0]   # y = H - 1
    v[35] = [9.5, 0.0, 1.0]    # y = 0
    v[36] = [13.0, 9.0, 1.0]   # isolated: named by no face
    v[37] = [2.0, 14.0, -3.0]
    v[38] = [20.0, 3.0, 2.0]
    v[39] = [17.0, 16.0, 0.5]
    faces = [[0, 1, 7], [1, 8, 7], [2, 3, 9], [3, 10, 9], [4, 5, 11], [5, 6, 11], [12, 13, 19], [13, 20, 19],
             [14, 15, 21], [15, 22, 21], [16, 17, 23], [17, 18, 23], [24, 25, 26], [27, 28, 29], [5, 5, 6], [30, 1, 2],
             [31, 2, 3], [32, 3, 4], [33, 34, 35], [37, 38, 39], [38, 37, 39], [0, 6, 18], [9, 9, 9], [10, 11, 37]]
    faces = np.array(faces, np.int64)
    m = 220
    verts = np.empty((m, 3), np.int64)
    bary = np.empty((m, 3), np.float64)
    for i in range(m):
        kind = i % 4
        if kind == 0:  # a vertex itself: the point is the vertex (half-integers, bounds, NaN, inf, the isolated one)
            j = i // 4 % n
            verts[i] = [j, (j + 1) % n, (j + 2) % n]
            bary[i] = [1.0, 0.0, 0.0]
        else:
            verts[i] = faces[rng.integers(0, len(faces))]
            r = rng.random(3) + 0.02
            bary[i] = r / r.sum()
    x_coords = rng.integers(-ADV_S, ADV_S, ADV_S * ADV_S).astype(np.float64)
    y_coords = rng.integers(-ADV_S, ADV_S, ADV_S * ADV_S).astype(np.float64)
    x_coords[::3] += 0.7  # truncated by astype(int), toward zero
    y_coords[1::4] -= 0.4
    x_coords = np.clip(x_coords, -ADV_S + 0.3, ADV_S - 0.3)
    y_coords = np.clip(y_coords, -ADV_S + 0.3, ADV_S - 0.3)
    ids = rng.integers(0, ADV_S * ADV_S, m).astype(np.int64)
    ids[m // 2:] = ids[rng.integers(0, m // 2, m - m // 2)]  # the second half lands on texels the first half uses
    td = {"x_coords": x_coords, "y_coords": y_coords, "valid_pixel_ids": ids, "valid_pixel_3d_faces": verts,
          "valid_pixel_b_coords": bary, "img_size": ADV_S}
    return v, faces, td


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dad_3dheads_amd import synthetic
    from oracle import flame_ref, reference_runner
    import uv_texture_restatement as R

    static = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, static)
    consts = flame_ref.FlameConstants.from_model(model)
    params = torch.from_numpy(synthetic.synthetic_params(4, seed=31))
    verts = flame_ref.reprojected_vertices(consts, params.clone(), to_2d=False).numpy().astype(np.float32)
    verts[:, :, 0] -= SHIFT_X
    verts[3, :, 2] *= -1.0
    with np.load(os.path.join(HERE, "demo_image.npz")) as z:
        photo = z["resized"]

    # the reference's module, unmodified, with its two third-party imports stood in for
    reference_runner.stand_in("psbody")
    psmesh = reference_runner.stand_in("psbody.mesh", Mesh=R.RestatedMesh)
    reference_runner.stand_in("model_training")
    reference_runner.stand_in("model_training.head_mesh", HeadMesh=object)
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from inference.uv_texture import UVTextureCreator

    recipes = [(256, 0, 0), (256, 0, 0), (256, 1, 4000), (256, 0, 0)]
    atlases = {}
    textures, digests = [], []
    for i, (s, seed, dups) in enumerate(recipes):
        key = (s, seed, dups)
        if key not in atlases:
            atlases[key] = synthetic.synthetic_texture_data(s, seed=seed, static=static, duplicates=dups)
        td = atlases[key]
        creator = object.__new__(UVTextureCreator)
        creator.texture_data = td
        tex = creator._compute_texture_map(photo, psmesh.Mesh(verts[i], static["faces"]))
        assert tex.dtype == np.uint8 and tex.shape == (s, s, 3)
        assert np.array_equal(tex, R.compute_texture_map(td, photo, verts[i], static["faces"])), i
        textures.append(tex)
        digests.append(synthetic.texture_data_digest(td))
        print(f"item {i}: S {s} seed {seed} dups {dups}: {int((tex.any(-1)).sum())} texels written")

    adv_v, adv_f, adv_td = adversarial()
    crop = np.ascontiguousarray(photo[:ADV_H, :ADV_W])
    creator = object.__new__(UVTextureCreator)
    creator.texture_data = adv_td
    adv_tex = creator._compute_texture_map(crop, psmesh.Mesh(adv_v, adv_f))
    assert np.array_equal(adv_tex, R.compute_texture_map(adv_td, crop, adv_v, adv_f))
    print(f"adv: {int((adv_tex.any(-1)).sum())} texels written")

    np.savez_compressed(
        OUT, verts=verts, textures=np.stack(textures), params=params.numpy(), shift_x=np.float32(SHIFT_X),
        flip_z=np.array([0, 0, 0, 1], np.int8), atlas_size=np.array([r[0] for r in recipes], np.int64),
        atlas_seed=np.array([r[1] for r in recipes], np.int64), atlas_duplicates=np.array([r[2] for r in recipes], np.int64),
        atlas_sha256=np.array(digests), adv_verts=adv_v, adv_faces=adv_f, adv_x_coords=adv_td["x_coords"],
        adv_y_coords=adv_td["y_coords"], adv_valid_pixel_ids=adv_td["valid_pixel_ids"],
        adv_valid_pixel_3d_faces=adv_td["valid_pixel_3d_faces"], adv_valid_pixel_b_coords=adv_td["valid_pixel_b_coords"],
        adv_img_size=np.int64(ADV_S), adv_crop_hw=np.array([ADV_H, ADV_W], np.int64), adv_texture=adv_tex,
        model_digest=np.array(synthetic.model_digest(model)))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
