#!/usr/bin/env python3
"""tests/golden/train_objective_edges_golden.npz: the reference's OWN `HeatmapCoder` at heatmap sizes whose plane is no multiple of a
16-byte chunk (S = 3, 5, 9, 25), made as make_train_objective_golden.py makes its coder cases: `raw` from the coder per item, `uint8` as
the dataset stores it, `float` as `uint8_to_float32` reads it. Inputs are `boundary_keypoints` (tests/train_objective_restatement.py)
at the sizes of tests/train_objective_cases.py. Data only, compressed.
Authoring container only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "train_objective_edges_golden.npz")


def main():
    import make_train_objective_golden as base
    import train_objective_cases as tc
    import train_objective_restatement as rs
    from dad_3dheads_amd import synthetic

    R = base.load_reference(synthetic.synthetic_flame_model(0, synthetic.load_static()))
    out = {}
    for i, (name, img, stride, radius) in enumerate(tc.ENCODE_SIZES):
        kp, pr = rs.boundary_keypoints(img // stride, stride, radius, seed=300 + i, n_random=6 + i % 5)  # C = 28 .. 32
        coder = R.coder.HeatmapCoder({"img_size": img, "stride": stride, "radius": radius}, kp.shape[1])
        raw = np.stack([coder(kp[b], pr[b]) for b in range(kp.shape[0])])
        u8 = np.uint8(255.0 * raw)  # flame_dataset.py:198
        f = R.flame.uint8_to_float32(torch.from_numpy(u8)).numpy()
        out.update({f"coder_{name}_keypoints": kp, f"coder_{name}_presence": pr, f"coder_{name}_raw": raw,
                    f"coder_{name}_uint8": u8, f"coder_{name}_float": f})
    out["coder_cases"] = np.array([f"{n}:{i}:{s}:{r}" for n, i, s, r in tc.ENCODE_SIZES])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
