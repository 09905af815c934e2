#!/usr/bin/env python3
"""Heatmap peaks and the point readjustment (dad-3dheads_amd/heatmap_points.py, csrc/heatmap_points.hip) on one MI355X beside the
framework chain they replace in the predictor, in the same process. Not collected by pytest.

C = 68; B = 64 and B = 1; 64 x 64 and 128 x 128; float32 channels-last (what InferenceNet returns) and bf16 NCHW (a plain module).
  heatmap_peaks_s        `heatmap_peaks(x, sigmoid=True)` (CUDA events, after warm-up)
  points_from_heatmap_s  `points_from_heatmap(x, geometry, 256, stride)`: the peaks and the readjustment, the geometry a device tensor
  torch_chain_s          the predictor's former chain on the device: sigmoid, view, argmax, div, mod, stack, flip, the product
  torch_chain_cpu_s      the same with its `.cpu()` behind it (host clock around a loop: every call waits for the device)
  heatmap_bytes          what the kernel reads: every logit once
  heatmap_peaks_gbps     heatmap_bytes / heatmap_peaks_s, a call's rate (launch included), not a kernel's share of peak
Every time is the median of five repeats of its loop; `*_spread_s` is the largest minus the smallest of the five. The numbers are
recorded as measured; no condition is asserted on them.

    python tests/perf/bench_heatmap_points.py [--out profiles/heatmap_points_bench.json]
"""
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, heatmap_points as hp  # noqa: E402
from event_timer import event_time  # noqa: E402


def torch_chain(x, stride):
    hm = torch.sigmoid(x).detach()
    b, c, h, w = hm.shape
    flat = hm.view(b, c, -1).argmax(-1) if hm.is_contiguous() else hm.reshape(b, c, -1).argmax(-1)
    yx = torch.stack((torch.div(flat, h, rounding_mode="trunc"), flat % h), dim=-1)
    return float(stride) * yx.flip(-1)


def host_time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def repeated(res, name, timer, fn, iters):
    times = sorted(timer(fn, iters, 10) for _ in range(5))
    res[name], res[name[:-2] + "_spread_s"] = times[2], times[4] - times[0]


def measure(batch, size, dtype, channels_last, iters):
    g = torch.Generator().manual_seed(size + batch)
    x = (4.0 * torch.randn(batch, 68, size, size, generator=g)).to(dtype).cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    stride = 256 // size
    geometry = torch.tensor([[32.0, 0.0, 256 / 683.0]] * batch, dtype=torch.float64).cuda()
    want = torch_chain(x, stride)
    got = float(stride) * hp.heatmap_peaks(x, sigmoid=True).flip(-1)
    n_bytes = x.numel() * x.element_size()
    res = {"B": batch, "shape": [68, size, size], "dtype": str(dtype).replace("torch.", ""), "layout": "channels_last" if channels_last else "nchw",
           "equal_to_torch_chain": bool(torch.equal(got, want)), "heatmap_bytes": n_bytes}
    repeated(res, "heatmap_peaks_s", event_time, lambda: hp.heatmap_peaks(x, sigmoid=True), iters)
    repeated(res, "points_from_heatmap_s", event_time, lambda: hp.points_from_heatmap(x, geometry, 256, stride), iters)
    repeated(res, "torch_chain_s", event_time, lambda: torch_chain(x, stride), iters)
    repeated(res, "torch_chain_cpu_s", host_time, lambda: torch_chain(x, stride).cpu(), iters)
    res["heatmap_peaks_gbps"] = n_bytes / res["heatmap_peaks_s"] * 1e-9
    res["speedup_vs_torch_chain"] = res["torch_chain_s"] / res["heatmap_peaks_s"]
    return res


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    runs = [measure(b, size, dtype, cl, iters=300) for b in (64, 1) for size in (64, 128)
            for dtype, cl in ((torch.float32, True), (torch.bfloat16, False))]
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "runs": runs}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
