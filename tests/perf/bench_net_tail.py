#!/usr/bin/env python3
"""The forward's tail (csrc/net_tail.hip) on one MI355X beside the framework chains it replaces, in the same process. Not collected
by pytest.

bf16, `DAD3DNet(seed=0)` as InferenceNet serves it, the tensors of a 256 x 256 input, B = 1, 64 and 256. Each piece against the
chain `tail="framework"` runs (network.py `DAD3DNet.forward`):
  fusion_in    interpolate (bilinear, align_corners) -> sigmoid -> cat                      vs  _glue.fusion_concat
  fusion_out   the 1x1 convolution with its bias, `* x`                                      vs  the convolution without it, _glue.bias_mul_
  heads        three means, six Linear, ReLUs, tanh * limit, relu, cat, .float()            vs  _glue.RegressionHeads
then the whole forward both ways: eager at B = 64 and from a graph at B = 1. Device timers (CUDA events around a loop, after warm-up);
every time is the median of five repeats, `*_spread_s` the largest minus the smallest. `faster` is the rule of the README row:
the framework's median exceeds this library's by more than the sum of the two spreads, at B = 1 or at B = 64.
`tanhf_sweep`: the device library's tanhf, through the heads' own kernel, over every float32 in [-9.1, 9.1] of stride 4099 bit
patterns against float64 tanh: the largest error in units of the last place (tests/net_tail_restatement.py reads it from the
recorded file).

    python tests/perf/bench_net_tail.py [--json profiles/net_tail_bench.json] [--pieces-only]
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import net_tail_restatement as T  # noqa: E402
from dad_3dheads_amd import _glue, _lib  # noqa: E402
from dad_3dheads_amd.network import HIP_TAIL_PIECES, DAD3DNet, GraphedNet, InferenceNet  # noqa: E402
from event_timer import event_time  # noqa: E402


def repeated(res, name, fn, iters):
    times = sorted(event_time(fn, iters, 10) for _ in range(5))
    res[name + "_s"], res[name + "_spread_s"] = times[2], times[4] - times[0]


def versus(res, piece, framework, hip, iters):
    repeated(res, piece + "_framework", framework, iters)
    repeated(res, piece + "_hip", hip, iters)
    gap = res[piece + "_framework_s"] - res[piece + "_hip_s"]
    res[piece + "_speedup"] = res[piece + "_framework_s"] / res[piece + "_hip_s"]
    res[piece + "_faster"] = bool(gap > res[piece + "_framework_spread_s"] + res[piece + "_hip_spread_s"])


def pieces(net, batch, iters):
    dad = net.net
    g = torch.Generator().manual_seed(batch)
    cl = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
    x, heat, level, top = cl(batch, 1024, 16, 16), cl(batch, 68, 64, 64), cl(batch, 256, 16, 16), cl(batch, 2048, 8, 8)
    fusion_in = _glue.fusion_concat(x, heat, level)
    heads = _glue.RegressionHeads((dad.shape, dad.pose, dad.landmarks), dad.limit_value)
    res = {"B": batch}

    def heads_framework():
        shape = torch.tanh(dad.shape(top)) * dad.limit_value
        lmk = F.relu(dad.landmarks(top)).reshape(batch, -1, 2)
        return torch.cat([shape, dad.pose(top)], dim=1).float(), lmk.float()

    with torch.no_grad():
        versus(res, "fusion_in", lambda: torch.cat([x, F.interpolate(heat, size=x.shape[2:], mode="bilinear", align_corners=True).sigmoid(), level], dim=1),
               lambda: _glue.fusion_concat(x, heat, level), iters)
        versus(res, "fusion_out", lambda: dad.fusion(fusion_in) * x, lambda: _glue.bias_mul_(F.conv2d(fusion_in, dad.fusion.weight), dad.fusion.bias, x), iters)
        versus(res, "heads", heads_framework, lambda: heads(top), iters)
    res["fusion_in_bytes"] = sum(t.numel() * 2 for t in (x, level, fusion_in)) + heat.numel() * 2
    res["heads_bytes"] = top.numel() * 2 + sum(p.numel() * 2 for m in (dad.shape, dad.pose, dad.landmarks) for p in m.parameters())
    return res


def forwards(batch, graph, iters):
    res = {"B": batch, "graph": graph}
    x = torch.randn(batch, 3, 256, 256, generator=torch.Generator().manual_seed(7)).cuda()
    fns = {}
    for tail in ("framework", "hip"):
        net = InferenceNet(DAD3DNet(seed=0), dtype=torch.bfloat16, tail=tail).cuda()
        fns[tail] = GraphedNet(net) if graph else net
    versus(res, "forward", lambda: fns["framework"](x), lambda: fns["hip"](x), iters)
    return res


def tanh_sweep():
    x = torch.from_numpy(T.tanh_sweep_inputs())
    n = x.numel()
    top = torch.zeros(1, 4, 1, 1, device="cuda").contiguous(memory_format=torch.channels_last)
    out = torch.empty(1, n, device="cuda")
    w1, b1, w2 = torch.zeros(4, 4, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(n, 4, device="cuda")
    _glue.regression_heads(top, [(w1, b1, w2, x.cuda(), T.ACT_TANH, 1.0, out, 0)])
    return {"values": n, "range": [-9.1, 9.1], "stride_bit_patterns": 4099,
            "max_ulp_error": T.ulp_error(out.cpu().numpy()[0], np.tanh(x.numpy().astype(np.float64)))}


def main():
    argv = sys.argv[1:]
    flag = "--out" if "--out" in argv else "--json"
    out = argv[argv.index(flag) + 1] if flag in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "dtype": "bfloat16",
           "tanhf_sweep": tanh_sweep(), "hip_tail_pieces": sorted(HIP_TAIL_PIECES)}
    net = InferenceNet(DAD3DNet(seed=0), dtype=torch.bfloat16).cuda()
    res["pieces"] = [pieces(net, b, iters=200 if b <= 64 else 50) for b in (1, 64, 256)]
    by_b = {p["B"]: p for p in res["pieces"]}
    res["faster_at_1_or_64"] = {k: bool(by_b[1][k + "_faster"] or by_b[64][k + "_faster"]) for k in ("fusion_in", "fusion_out", "heads")}
    if "--pieces-only" not in argv:
        res["forward"] = [forwards(64, False, 20), forwards(1, True, 200)]
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
