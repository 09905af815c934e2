#!/usr/bin/env python3
"""The piece-wise entropy stage of the JPEG reader (csrc/jpeg_decode_sync.hip) beside the one-lane-per-segment
decoder (dad3d_jpeg_decode, untouched: the yardstick) and beside PIL on one core, in the same process. Not collected by pytest.

The two forms of tests/perf/bench_jpeg_decode.py: 64 files of 512 x 512 x 3 at 4:2:0 and quality 90, without restart markers and
with `restart_marker_rows=1`. Per form, after every device result has been compared with PIL:
  pil_s                    `np.asarray(Image.open(f).convert("RGB"))` of all 64 on one core (host clock, best of 3)
  segments / sync_<P>      the launches of dad3d_jpeg_decode and of dad3d_jpeg_decode_sync at pieces of P = 64, 128, 256 bytes with the
                           file bytes already on the device: five repeats of the event-timed loop each (seconds per call), their
                           median and their spread (largest minus smallest)
  decode_call_s            `JpegDecoder(entropy=...).decode` end to end (host clock, best of 3)
Required, and the process fails where it does not hold: without restart markers "sync" at its default piece size is faster than
"segments" by more than the spread of the five repeats (the larger of the two spreads); with restart markers it is no slower beyond
that spread. How it stands against PIL is reported only. Hand-over rounds per file are not reported: the kernels do not count them.

    python tests/perf/bench_jpeg_decode_sync.py [--out profiles/jpeg_decode_sync_bench.json]
"""
import io
import json
import os
import statistics
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from dad_3dheads_amd import _lib, jpeg_reader  # noqa: E402
from bench_jpeg_decode import SIDE, Plan, host_clock, photos, pil_decode  # noqa: E402
from event_timer import event_time  # noqa: E402

PIECES = (64, 128, 256)
REPEATS = 5


class SyncPlan(Plan):
    """The buffers of one dad3d_jpeg_decode_sync call, allocated once."""

    def __init__(self, files, piece_bytes):
        super().__init__(files)
        self.piece_bytes = piece_bytes
        desc = np.concatenate([self.desc.cpu().numpy().ravel(), np.zeros(4 * self.n, np.int64)])
        self.grid = np.zeros(_lib.JPEG_DECODE_SYNC_GRID_INTS, dtype=np.int32)
        self.scratch_bytes = self.lib.dad3d_jpeg_decode_sync_scratch_bytes(desc.ctypes.data, self.n, self.grid.ctypes.data, piece_bytes)
        assert self.scratch_bytes > 0
        self.desc = torch.from_numpy(desc).cuda()
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device="cuda")
        self.info = torch.empty((self.n, 4), dtype=torch.int32, device="cuda")

    def launch(self):
        _lib.check(self.lib.dad3d_jpeg_decode_sync(self.data.data_ptr(), self.file_bytes, self.desc.data_ptr(), self.n, self.grid.ctypes.data,
                                                   self.piece_bytes, self.out.data_ptr(), self.out_bytes, self.flags.data_ptr(),
                                                   self.info.data_ptr(), self.scratch.data_ptr(), self.scratch_bytes, 0,
                                                   torch.cuda.current_stream().cuda_stream))


def repeats(plan, want):
    plan.out.zero_()
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.flags.cpu().any()
    assert np.array_equal(plan.out.view(plan.n, SIDE, SIDE, 3).cpu().numpy(), want)  # against PIL, before any timing
    times = [event_time(plan.launch, 3, 1) for _ in range(REPEATS)]
    return {"repeats_s": times, "median_s": statistics.median(times), "spread_s": max(times) - min(times)}


def measure(name, files, want):
    run = {"form": name, "file_bytes": sum(map(len, files)), "segments_per_file": 1 + sum(files[0].count(bytes([0xFF, 0xD0 + k])) for k in range(8)),
           "pil_s": host_clock(lambda: pil_decode(files), 3), "segments": repeats(Plan(files), want)}
    for p in PIECES:
        plan = SyncPlan(files, p)
        run[f"sync_{p}"] = repeats(plan, want)
        run[f"sync_{p}"]["modes"] = sorted(set(plan.info[:, 0].cpu().tolist()))
        run[f"sync_{p}"]["groups_per_file"] = int(plan.info[:, 2].max())
    for entropy in jpeg_reader.ENTROPY:
        decoder = jpeg_reader.JpegDecoder(0, entropy=entropy)
        res = decoder.decode(files, channels=3)
        assert not res.flags.any() and all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(res.tensors(), want))
        run[f"decode_call_{entropy}_s"] = host_clock(lambda: decoder.decode(files, channels=3), 3)
    default = run[f"sync_{jpeg_reader.SYNC_PIECE_BYTES}"]
    run["spread_s"] = max(default["spread_s"], run["segments"]["spread_s"])
    run["speedup_over_segments"] = run["segments"]["median_s"] / default["median_s"]
    run["speedup_over_pil"] = run["pil_s"] / default["median_s"]
    return run


def main():
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    _lib.require_gpu()
    torch.cuda.set_device(0)
    images = photos()
    runs = []
    for name, options in (("no restart markers", {}), ("restart_marker_rows=1", {"restart_marker_rows": 1})):
        files = []
        for img in images:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=90, subsampling=2, **options)
            files.append(buf.getvalue())
        runs.append(measure(name, files, np.stack(pil_decode(files))))
    default = f"sync_{jpeg_reader.SYNC_PIECE_BYTES}"
    plain, marked = runs
    fastest = min(PIECES, key=lambda p: plain[f"sync_{p}"]["median_s"])
    required = {"without markers sync is faster than segments by more than the spread":
                plain["segments"]["median_s"] - plain[default]["median_s"] > plain["spread_s"],
                "with markers sync is no slower than segments beyond the spread":
                marked[default]["median_s"] - marked["segments"]["median_s"] <= marked["spread_s"]}
    res = {"device": torch.cuda.get_device_name(0), "build": _lib.load().dad3d_build_info().decode(), "batch": len(images), "shape": [SIDE, SIDE, 3],
           "quality": 90, "subsampling": "4:2:0", "default_piece_bytes": jpeg_reader.SYNC_PIECE_BYTES, "fastest_piece_bytes": fastest,
           "required": required, "not_measured": ["hand-over rounds per file"], "runs": runs}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not all(required.values()):
        sys.exit("a required condition does not hold: " + ", ".join(k for k, v in required.items() if not v))


if __name__ == "__main__":
    main()
