#!/usr/bin/env python3
"""Build tests/golden/lmk68_embedding.npz: the 68-landmark barycentric embedding of the FLAME topology and golden
outputs of the reference's OWN `get_68_landmarks` (dad_3dheads_benchmark/utils.py:99-117 == model_training/data/utils.py:
188-204), executed unmodified from where it lies.

Runs ONLY in the authoring container (needs /root/reference). The two imports that are not installed, `cv2` (never called
on this path) and `smplx` (`Struct` and the zero-pose `find_dynamic_lmk_idx_and_bcoords`, PARITY UNPINNED), are the
stand-ins of oracle/reference_runner.py.

  face_idx   int64 [68]     dynamic row 0 (17 contour points) then the 51 static points
  b_coords   f32   [68,3]
  verts      f32   [3,5023,3] seeded test meshes          lmk68  f32 [3,68,3] = reference get_68_landmarks(verts[i])
The tables are (c) the FLAME / DAD-3DHeads authors (see NOTICE.md); data, not code.
"""
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import reference_runner  # noqa: E402

BENCH = os.path.join(reference_runner.REFERENCE_ROOT, "dad_3dheads_benchmark")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "lmk68_embedding.npz")


def main():
    reference_runner.install_stand_ins()
    sys.dont_write_bytecode = True
    sys.path.insert(0, BENCH)
    os.chdir(BENCH)  # the reference opens "data/static/..." relative to its own directory
    import utils as ref_utils  # dad_3dheads_benchmark/utils.py

    dyn = np.load("data/static/flame_dynamic_embedding.npy", allow_pickle=True, encoding="latin1")[()]
    with open("data/static/flame_static_embedding.pkl", "rb") as f:
        sta = pickle.load(f, encoding="latin1")
    face_idx = np.concatenate([np.array(dyn["lmk_face_idx"]).astype(np.int64)[0], sta["lmk_face_idx"].astype(np.int64)])
    b_coords = np.concatenate([np.array(dyn["lmk_b_coords"])[0], sta["lmk_b_coords"]]).astype(np.float32)
    assert face_idx.shape == (68,) and b_coords.shape == (68, 3)
    g = torch.Generator().manual_seed(68)
    verts = (torch.randn(3, 5023, 3, generator=g) * 0.1).float()
    lmk = torch.stack([ref_utils.get_68_landmarks(v) for v in verts])
    seven = np.stack([ref_utils.get_7_landmarks_from_68(l) for l in lmk])
    np.savez_compressed(OUT, face_idx=face_idx, b_coords=b_coords, verts=verts.numpy(), lmk68=lmk.numpy(), lmk7=seven)
    if len(sys.argv) <= 1:  # the embedding alone is package data (dad-3dheads_amd/assets/), the goldens stay here
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(OUT))))
        np.savez_compressed(os.path.join(root, "dad-3dheads_amd", "assets", "lmk68_embedding.npz"), face_idx=face_idx, b_coords=b_coords)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; lmk68", lmk.shape, "lmk7", seven.shape)


if __name__ == "__main__":
    main()
