#!/usr/bin/env python3
"""The device JSON reader (dad-3dheads_amd/json_reader.py, csrc/json_parse.hip) beside `json.loads` on the two documents DADEvaluator
reads, in one process on one MI355X. Not collected by pytest.

Documents: those of tests/perf/bench_eval.py (the three complete items of tests/golden/eval_golden.npz repeated to B), written in full:
B = 1024 is about 0.7 GB of text. Reported per B:
  bytes                both documents
  json_loads_s         json.loads of both documents (bytes in memory)
  reader_load_s        json_reader.load of both: pinned copy, H2D, kernels, list work, skeleton parse (synchronised, wall clock)
  reader_kernels_s     the four library entries alone (CUDA events around each call), summed over both documents
  h2d_s                the copy of both documents from pinned memory to the device (CUDA events)
  reader_lift_s        the device part without H2D and skeleton: kernels + list work + the reads of the counts and records
  evaluator_*_s        DADEvaluator(...)() end to end from the two files, reader="host" and reader="device"; items/s = B / that

    python tests/perf/bench_json_parse.py [B ...] [--out profiles/json_parse_bench.json]
"""
import json
import os
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import eval_restatement as er  # noqa: E402
from bench_eval import documents, items  # noqa: E402
from dad_3dheads_amd import _lib, evaluation, json_reader  # noqa: E402
from event_timer import event_time  # noqa: E402


def wall(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def run(golden, b, directory):
    repeats = 3 if b <= 256 else 1
    gt_text, sub_text = documents(golden, items(golden, b, seed=b))
    docs = [gt_text.encode(), sub_text.encode()]
    del gt_text, sub_text
    paths = [os.path.join(directory, "gt_%d.json" % b), os.path.join(directory, "submission_%d.json" % b)]
    for path, data in zip(paths, docs):
        with open(path, "wb") as f:
            f.write(data)
    json_reader.load(docs[1][:1] + b"}", device=0)  # library and allocator warm
    t_loads = wall(lambda: [json.loads(d) for d in docs], repeats)
    t_load = wall(lambda: [json_reader.load(d, device=0) for d in docs], repeats)
    lifted = [json_reader.load(d, device=0) for d in docs]
    n_values = sum(int(doc.values.numel()) for doc in lifted)
    del lifted
    t_lift, t_kernels, per_entry = 0.0, 0.0, {}
    t_h2d = 0.0
    for d in docs:
        pinned = json_reader._read(d)
        t_h2d += event_time(lambda: pinned.to("cuda:0", non_blocking=True), repeats, 1)
        text = pinned.to("cuda:0")
        t_lift += wall(lambda: json_reader.lift(text), repeats)
        events = []
        json_reader.lift(text, events=events)
        torch.cuda.synchronize()
        for name, e0, e1 in events:
            per_entry[name] = per_entry.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
        del text
    t_kernels = sum(per_entry.values())
    res = {"B": b, "bytes": sum(len(d) for d in docs), "lifted_values": n_values, "json_loads_s": t_loads, "reader_load_s": t_load,
           "h2d_s": t_h2d, "reader_lift_s": t_lift, "reader_kernels_s": t_kernels, "reader_entries_s": per_entry, "speedup_load": t_loads / t_load}
    del docs
    for reader in ("host", "device"):
        ev = evaluation.DADEvaluator(paths[0], paths[1], face_indices=golden["face_indices"], reader=reader)
        ev()  # warm: kernels, allocator, page cache
        out = []
        t = wall(lambda: out.append(ev()), 1)
        res["evaluator_%s_s" % reader] = t
        res["evaluator_%s_items_per_s" % reader] = b / t
        res["evaluator_%s_overall" % reader] = out[0][0]
    res["evaluator_results_equal"] = res["evaluator_host_overall"] == res["evaluator_device_overall"]
    for path in paths:
        os.remove(path)
    return res


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    sizes = [int(x) for x in argv] or [64, 1024]
    _lib.require_gpu()
    torch.cuda.set_device(0)
    golden = er.load_golden()
    with tempfile.TemporaryDirectory() as directory:
        res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(),
               "tile_bytes": _lib.JSON_PARSE_TILE_BYTES, "runs": [run(golden, b, directory) for b in sizes]}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
