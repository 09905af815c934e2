#!/usr/bin/env python3
"""The `.obj` vertex formatter (dad-3dheads_amd/writers.py `ObjFormatter`, csrc/obj_text.hip) on one MI355X beside the host
formatting it replaces (`np.savetxt` per mesh, `save_obj_batch(..., formatter="host")`), in the same process. Not collected by pytest.

Inputs: decoded synthetic meshes (`vertices_3d` of seeded params). Per batch size B:
  decode_s               the decode of the same batch (CUDA events), for scale
  format_kernels_s       the two format launches (CUDA events, after warm-up)
  text_bytes_per_mesh    mean length of a mesh's vertex block
  floor_s                (B * 5023 * 12 bytes read + the text bytes written) / 8 TB/s, and the fraction of it the kernels reach
  copy_to_pinned_s       lengths + flags, the dense repack and the copy of the text into pinned memory (host clock, synchronised)
  obj_text_batch_s       `obj_text_batch` end to end: format + copy + bytes objects with the face block appended (host clock)
  host_format_s          the parent's path to the same bytes: floats to the host, `_vertex_block` per mesh (host clock)
  speedup_format_copy    host_format_s / (format_kernels_s + copy_to_pinned_s)
  write_files_s          writing B ready blocks + the face block to a temporary directory: bound by the file system, the same
                         for both paths
  save_obj_batch_*_s     `save_obj_batch` whole, both ways

    python tests/perf/bench_obj_text.py [--out profiles/obj_text_bench.json] [--batches 64,256]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, synthetic, writers  # noqa: E402
from dad_3dheads_amd.head_mesh import HeadMesh  # noqa: E402
from event_timer import event_time  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def host_clock(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def run(hm, faces, b, iters):
    params = torch.from_numpy(synthetic.synthetic_params(b, seed=b)).cuda()
    verts = hm.flame.decode(params, verts3d=True)["verts3d"]
    n = verts.shape[1]
    fmt = writers.ObjFormatter(n, faces, device=0)
    fmt.reserve(b)
    t_decode = event_time(lambda: hm.flame.decode(params, verts3d=True), iters, 10)
    t_kernels = event_time(lambda: fmt.format(verts), iters, 10)
    text = fmt.format(verts)
    torch.cuda.synchronize()
    assert not text.flags.cpu().any()
    text_bytes = int(text.lengths.sum().item())

    def copy():
        text._copy = None
        text.begin_host_copy()
        text._copy[3].synchronize()

    copy()
    t_copy = host_clock(copy, 5)
    faces1 = faces + 1.0
    writers.obj_text_batch(verts, faces1)
    t_e2e = host_clock(lambda: writers.obj_text_batch(verts, faces1), 3)

    host_blocks = []

    def host_format():
        host_blocks[:] = [writers._vertex_block(row) for row in verts.detach().cpu().numpy()]

    t_host = host_clock(host_format, 1)
    blocks = [bytes(x) for x in text.to_host()]
    assert blocks == [h.encode("ascii") for h in host_blocks]  # the same bytes, at the size timed
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, f"{i}.obj") for i in range(b)]
        t_write = host_clock(lambda: writers._write_obj_files(blocks, fmt.face_text, paths), 3)
        t_save_gpu = host_clock(lambda: writers.save_obj_batch(verts, faces, paths), 2)
        t_save_host = host_clock(lambda: writers.save_obj_batch(verts, faces, paths, formatter="host"), 1)
    floor = (b * n * 12 + text_bytes) / HBM_BYTES_PER_S
    res = {"B": b, "n_verts": n, "decode_s": t_decode, "format_kernels_s": t_kernels, "text_bytes_per_mesh": text_bytes / b,
           "floor_s": floor, "fraction_of_floor": floor / t_kernels, "copy_to_pinned_s": t_copy, "obj_text_batch_s": t_e2e,
           "host_format_s": t_host, "speedup_format_copy": t_host / (t_kernels + t_copy), "speedup_obj_text_batch": t_host / t_e2e,
           "write_files_s": t_write, "save_obj_batch_gpu_s": t_save_gpu, "save_obj_batch_host_s": t_save_host}
    assert t_kernels + t_copy < t_host, res  # the one condition: format + copy beats the host formatting of the same batch
    return res


def main():
    argv = sys.argv[1:]
    out, batches = None, (64, 256)
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    if "--batches" in argv:
        i = argv.index("--batches")
        batches = tuple(int(x) for x in argv[i + 1].split(","))
        del argv[i:i + 2]
    _lib.require_gpu()
    torch.cuda.set_device(0)
    static = synthetic.load_static()
    hm = HeadMesh(flame_model=synthetic.synthetic_flame_model(0, static), static=static, device=0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
           "runs": [run(hm, static["faces"], b, iters=200) for b in batches]}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
