#!/usr/bin/env python3
"""The JSON formatter (dad-3dheads_amd/writers.py `JsonFormatter`, csrc/json_text.hip) on one MI355X beside the host formatting it
replaces, in the same process. Not collected by pytest.

Two layouts, seeded inputs (submission: normal vertices x 0.1, int32 2-D points; params: `synthetic_params`):
  submission, batch 64    host: `submission_entry` + `json.dumps` per image      device: `SubmissionFormatter.format` + copy to pinned
  flame params, batch 256 host: `json.dumps(get_flame_params(...))` per image    device: gather + `JsonFormatter.format` + copy to pinned
Per layout:
  host_s             the host path for the whole batch (host clock, one run: it takes about a second)
  format_kernels_s   the gather and the two format launches (CUDA events, after warm-up)
  copy_to_pinned_s   lengths + flags, the dense repack and the copy of the text into pinned memory (host clock, synchronised)
  device_s           format_kernels_s + copy_to_pinned_s
  text_bytes         bytes of the batch's text (the same on both paths: the bytes are compared)
The one condition: device_s < host_s for each layout.

    python tests/perf/bench_json_text.py [--out profiles/json_text_bench.json]
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
from dad_3dheads_amd import _lib, benchmark_export, synthetic, writers  # noqa: E402
from event_timer import event_time  # noqa: E402


def host_clock(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def measure(name, batch, launch, host_path, iters):
    """launch() -> JsonText on the current stream; host_path() -> list of bytes."""
    t_kernels = event_time(launch, iters, 10)
    text = launch()
    torch.cuda.synchronize()
    assert not text.flags.cpu().any()
    text_bytes = int(text.lengths.sum().item())

    def copy():
        text._copy = None
        text.begin_host_copy()
        text._copy[3].synchronize()

    copy()
    t_copy = host_clock(copy, 5)
    blocks = [bytes(x) for x in text.to_host()]
    host_blocks = []

    def run_host():
        host_blocks[:] = host_path()

    t_host = host_clock(run_host, 1)
    assert blocks == host_blocks  # the same bytes, at the size timed
    res = {"layout": name, "B": batch, "n_slots": text.formatter.n_slots, "text_bytes": text_bytes, "host_s": t_host,
           "format_kernels_s": t_kernels, "copy_to_pinned_s": t_copy, "device_s": t_kernels + t_copy, "speedup": t_host / (t_kernels + t_copy)}
    assert res["device_s"] < res["host_s"], res
    return res


def submission(batch, iters):
    rng = np.random.default_rng(batch)
    points = torch.from_numpy(rng.integers(0, 256, (batch, 68, 2)).astype(np.int32)).cuda()
    vertices = torch.from_numpy((rng.standard_normal((batch, 5023, 3)) * 0.1).astype(np.float32)).cuda()
    lmk68 = torch.from_numpy((rng.standard_normal((batch, 68, 3)) * 0.1).astype(np.float32)).cuda()
    rotation = torch.from_numpy(np.linalg.qr(rng.standard_normal((batch, 3, 3)))[0].astype(np.float32)).cuda()
    fmt = benchmark_export.SubmissionFormatter(device=0)
    fmt.reserve(batch)

    def host_path():
        return [json.dumps(benchmark_export.submission_entry(points[i], vertices[i], lmk68[i], rotation[i])).encode() for i in range(batch)]

    return measure("submission", batch, lambda: fmt.format(points, vertices, lmk68, rotation), host_path, iters)


def flame_params(batch, iters):
    params = torch.from_numpy(synthetic.synthetic_params(batch, seed=batch)).cuda()
    writers.flame_params_json_batch(params)  # builds and reserves the cached formatter

    def host_path():
        return [json.dumps(writers.get_flame_params({"3dmm_params": params[i:i + 1]})).encode() for i in range(batch)]

    return measure("flame_params", batch, lambda: writers._format_flame_params(params, writers.FLAME_CONSTS), host_path, iters)


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
           "runs": [submission(64, iters=100), flame_params(256, iters=200)]}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
