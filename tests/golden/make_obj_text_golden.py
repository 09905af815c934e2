#!/usr/bin/env python3
"""tests/golden/obj_text_golden.npz: the bytes the reference's OWN `demo_utils.MeshSaver` (demo_utils.py:130-144) writes for three
seeded float32 meshes, TOGETHER WITH those float32 inputs: the text does not determine the float, and a GPU decode differs from
the oracle's in the last bits, so a test of the GPU formatter (csrc/obj_text.hip) feeds the stored floats. Authoring container
only; `demo_utils` is imported unmodified from where it lies, the way make_writers_golden.py does.

  metre  5023 vertices in FLAME units: the oracle's `vertices_3d` of seeded params
  pixel  5023 vertices in pixels: its `reprojected_vertices(to_2d=False)` of the same row
  edge   the corners of the integer rule: +-0, +-1e-45, just below and at 5e-9, ties at the eighth decimal (odd / 2^9), odd / 2^12,
         0.99999999 and 0.999999995 (float32 rounds both to 1.0: the carry into a new digit happens in the conversion), the
         float32 neighbours below 1, 10, 1e5, 1e6 and around 1e11 (a change of the integer digit count), 9.9999999, 99999.999, negatives that round to zero, the largest
         float32 below 2^37 and seeded values of every magnitude in between
Every stored value lies inside the kernel's domain (finite, |x| < 2^37); asserted below. The face list handed to MeshSaver is two
faces long: the face block is not what this fixture pins (writers_golden.npz does)."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "obj_text_golden.npz")
SEED = 412


def edge_values():
    f32 = np.float32
    below_5e9 = np.nextafter(f32(5e-9), f32(0))
    top = np.nextafter(f32(2.0 ** 37), f32(0))
    v = [0.0, -0.0, 1e-45, -1e-45, below_5e9, f32(5e-9), -below_5e9, -f32(5e-9), np.nextafter(f32(5e-9), f32(1)),
         0.99999999, 0.999999995, -0.99999999, -0.999999995, 9.9999999, -9.9999999, 99999.999, -99999.999, 99.999999, 999999.99,
         -1e-9, -4e-9, -1e-20, 1e-20, 4.9e-9, 1.5e-8, 2.5e-8, top, -top, 2.0 ** 36, 2.0 ** 24, 2.0 ** 24 + 2, 1e10, 123456789.0,
         1.0, -1.0, 10.0, 100.0, 0.1, 0.5, 1.17549435e-38, 1e-38, np.nextafter(f32(1), f32(0)), np.nextafter(f32(10), f32(0)),
         np.nextafter(f32(1e5), f32(0)), np.nextafter(f32(1e6), f32(0)), np.nextafter(f32(1e11), f32(0)), np.nextafter(f32(1e11), f32(2e11))]
    v += [k / 512.0 for k in range(1, 129, 2)] + [-k / 512.0 for k in range(1, 33, 2)]   # exact ties at the eighth decimal
    v += [k / 4096.0 for k in range(1, 65, 2)] + [1234.0 + k / 512.0 for k in (1, 3, 5, 255, 511)]
    rng = np.random.default_rng(SEED)
    v += list((rng.standard_normal(120) * 10.0 ** rng.integers(-9, 11, 120)).astype(np.float32))
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([v, np.zeros((-len(v)) % 3, dtype=np.float32)]).reshape(-1, 3)


def main():
    from dad_3dheads_amd import synthetic
    from make_writers_golden import load_reference_demo_utils
    from oracle import flame_ref

    st = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, st)
    fc = flame_ref.FlameConstants.from_model(model)
    du = load_reference_demo_utils(model)
    params = torch.from_numpy(synthetic.synthetic_params(1, seed=SEED))
    meshes = {"metre": flame_ref.vertices_3d(fc, params.clone())[0].numpy(),
              "pixel": flame_ref.reprojected_vertices(fc, params.clone(), to_2d=False)[0].numpy(),
              "edge": edge_values()}
    faces = st["faces"][:2] + 1.0
    out = {"seed": SEED, "names": np.array(list(meshes))}
    with tempfile.TemporaryDirectory() as d:
        for name, v in meshes.items():
            v = np.ascontiguousarray(v, dtype=np.float32)
            assert v.ndim == 2 and v.shape[1] == 3
            assert np.isfinite(v).all() and (np.abs(v.astype(np.float64)) < 2.0 ** 37).all(), f"{name}: outside the kernel's domain"
            path = os.path.join(d, name + du.MeshSaver().extension)
            du.MeshSaver()((v, faces), path)
            out[f"vertices_{name}"] = v
            out[f"obj_{name}"] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    assert np.abs(meshes["metre"]).max() < 1.0 < np.abs(meshes["pixel"]).max()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {n: (len(out[f"vertices_{n}"]), out[f"obj_{n}"].size) for n in meshes})


if __name__ == "__main__":
    main()
