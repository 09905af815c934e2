#!/usr/bin/env python3
"""tests/golden/writers_golden.npz: the bytes the reference's OWN `demo_utils.py` writes (MeshSaver / JsonSaver /
get_flame_params / get_mesh / get_output_path, demo_utils.py:106-163), imported unmodified from where it lies.
Authoring container only. Stand-ins are registered for the imports this path never calls (cv2, the two `inference`
modules, `model_training.utils`); `utils.get_relative_path` comes from the reference itself; `model_training.model.flame`
is loaded the way oracle/reference_runner.py loads it. `get_mesh` reads 'model_training/model/static/flame_mesh_faces.pt'
relative to the working directory: the script runs from the reference root, so that is the reference's own file.
Inputs are seeded (vertices: a decode of seeded params through the oracle; params: the same rows), so only bytes travel."""
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "writers_golden.npz")
SEED, BATCH = 205, 2


def load_reference_demo_utils(model):
    from oracle import reference_runner as rr

    rr.load_reference_head_mesh(model)  # the shared stand-ins (cv2 among them), sys.path, patched get_flame_model
    rr.stand_in("inference")
    rr.stand_in("inference.uv_texture", UVTextureCreator=type("UVTextureCreator", (), {}))
    rr.stand_in("inference.pncc_estimator", PNCCEstimator=type("PNCCEstimator", (), {}))
    rr.stand_in("model_training.utils", load_indices_from_npy=lambda p: np.load(p))  # only a name is needed
    import importlib

    return importlib.import_module("demo_utils")


def main():
    from dad_3dheads_amd import synthetic
    from oracle import flame_ref, reference_runner as rr

    st = synthetic.load_static()
    model = synthetic.synthetic_flame_model(0, st)
    fc = flame_ref.FlameConstants.from_model(model)
    os.chdir(rr.REFERENCE_ROOT)  # get_mesh's relative torch.load
    du = load_reference_demo_utils(model)
    params = torch.from_numpy(synthetic.synthetic_params(BATCH, seed=SEED))
    verts = flame_ref.vertices_3d(fc, params.clone())
    out = {"seed": SEED, "batch": BATCH}
    with tempfile.TemporaryDirectory() as d:
        for i in range(BATCH):
            pred = {"3d_vertices": verts[i], "3dmm_params": params[i : i + 1]}
            mesh = du.get_mesh(pred)
            fl = du.get_flame_params(pred)
            po, pj = os.path.join(d, f"m{i}.obj"), os.path.join(d, f"m{i}.json")
            du.MeshSaver()(mesh, po)
            du.JsonSaver()(fl, pj)
            out[f"obj_{i}"] = np.frombuffer(open(po, "rb").read(), dtype=np.uint8)
            out[f"json_{i}"] = np.frombuffer(open(pj, "rb").read(), dtype=np.uint8)
            if i == 0:
                out["faces_plus_one_dtype"] = np.array(str(mesh[1].dtype))
                out["faces_equal_static"] = np.array(bool(np.array_equal(mesh[1], st["faces"] + 1.0)))
    out["output_path"] = np.array(du.get_output_path("/data/in/some.image.jpeg", "outputs", "head_mesh", du.MeshSaver().extension))
    out["extensions"] = np.array([du.ImageSaver().extension, du.MeshSaver().extension, du.JsonSaver().extension])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; obj", out["obj_0"].size, "json", out["json_0"].size, "faces == static:", out["faces_equal_static"])


if __name__ == "__main__":
    main()
