#!/usr/bin/env python3
"""Phase breakdown of the pipelined decode kernel (flame_decode_pipe.hip) from its in-kernel shader-clock stamps (diagnostics).

    python tools/trace_pipe.py [batch]

Slots, both roles: 0 start | 5 end | 12, 13 wall clock (100 MHz) | 6, 7 at / past the first barrier (stagers: 7 = first part of A(0) published).
mma waves: 16 basis requests issued = first GEMM start | 1, 4 constants round 0 begun / written and announced | 2 first GEMM done | 3 last barrier passed.
stager waves: 1 first loads issued | 2 A(0) published (3, 4: constants round 0 begun / written, only in profiles/r08_round0_in_stagers_experiment.patch).
First four half-blocks h: 16+4h before the GEMM / phase start, 17+4h accumulators parked / A(h+1) written, 18+4h past the barrier / next loads
issued, 19+4h (stagers) past the barrier.
(Builds before profiles/r08_kernel_log.md wrote the round between groups 6 and 7 of the first GEMM, in front of a barrier of its own: there slot 1
is also "first seven MFMA groups done". Launches of one half-block still do. A slot a build does not stamp prints as n/a.)
Whole-mesh launches of 33..64 rows take flame_decode_head.hip (48 rows under the basis stream, then 16; DAD3D_DECODE_KERNEL=halfblocks: the two
half-blocks above). Same slots: 16 up-front basis requests issued | 8 first MFMA | 2, 17 pass 1 multiplied, parked | 18 past barrier P1 |
20, 21 pass 2 start, parked | 22, 3 past barrier P2. Stagers: 16, 17 rows 48..63 requested, written | 18, 19 at / past P1 | 21 rows 32..47
finished | 23 past P2. The half-block lines below then read: half-block 0 = pass 1, half-block 1 = pass 2.
The seam experiment (profiles/r12_seam_experiment.patch, no barrier P1 at B > 48) keeps the slots usable: mma waves 20 = behind the chain's
first MFMA | 17 = pass 1 parked and announced (behind the chain's fourth MFMA) | 18 = `parked` seen full, in front of the hooks' first fetch;
stagers 17 = rows 48..63 written and announced | 18, 19 = in front of / behind the wait for `parked`.
Stagers, B > 48: 9 = vertices 16..19 of rows 0..31 finished (behind slot 21). The ride experiment (profiles/r11_ride_experiment.patch) uses
9, 10 differently: mma waves 9 = k 0..127 of rows 48..63 seen in LDS; stagers 9, 10 = k 0..127, k 128..255 of rows 48..63 published."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dad_3dheads_amd import _lib, landmarks, synthetic  # noqa: E402
from dad_3dheads_amd.head_mesh import HeadMesh  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 64
st = synthetic.load_static()
hm = HeadMesh(flame_model=synthetic.synthetic_flame_model(0, st), landmarks=landmarks.canonical("445", st), static=st, device=0)
p = torch.from_numpy(synthetic.synthetic_params(batch, seed=0)).cuda()
tiles = 252
trace = torch.zeros((4096, 32), dtype=torch.int64, device="cuda")
lib = _lib.load()
v3 = torch.empty((batch, 5023, 3), device="cuda"); pr = torch.empty((batch, 5023, 2), device="cuda"); lp = torch.empty((batch, 445, 2), dtype=torch.int32, device="cuda")
call = (hm.flame._handle, p.data_ptr(), batch, _lib.TO_2D, v3.data_ptr(), pr.data_ptr(), None, lp.data_ptr(), None)
for _ in range(200):
    lib.dad3d_flame_decode(*call)
hm.flame.select_kernel("pipelined")  # these stamps are the pipelined kernel's layout
_lib.check(lib.dad3d_flame_debug_trace(hm.flame._handle, trace.data_ptr(), trace.numel()))
_lib.check(lib.dad3d_flame_decode(*call))
torch.cuda.synchronize()
_lib.check(lib.dad3d_flame_debug_trace(hm.flame._handle, None, 0))
t = trace.cpu().numpy().astype(np.float64)[: tiles * 8].reshape(tiles, 8, 32)
rel = t - t[:, :, 0:1]
wall = (t[:, :, 13] - t[:, :, 12]) / 100.0
clk = (t[:, 0, 5] - t[:, 0, 0]) / wall[:, 0]
print(f"batch {batch}: wave lifetime {np.median(wall[:, :4]):.2f} us (mma) {np.median(wall[:, 4:]):.2f} us (stagers); shader clock {np.median(clk):.0f} MHz; "
      f"workgroup start spread {(t[:, 0, 12].max() - t[:, 0, 12].min()) / 100.0:.2f} us")
def med(w, slot):
    return float(np.median(rel[:, w, slot])) if t[:, w, slot].any() else float("nan")
def cyc(x):
    return "n/a" if np.isnan(x) else f"{x:.0f}"
print("mma waves (cycles since wave start, median over tiles; wave 0 / wave 3):")
print(f"  at the first barrier {med(0, 6):.0f} / {med(3, 6):.0f}, past it {med(0, 7):.0f} / {med(3, 7):.0f}, basis requests issued {med(0, 16):.0f} / {med(3, 16):.0f}")
print(f"  constants round 0 begun (builds before r08: = first seven MFMA groups done) {med(0, 1):.0f} / {med(3, 1):.0f}; constants round 0 written by the mma waves {cyc(med(0, 4))} / {cyc(med(3, 4))}; "
      f"first GEMM done {med(0, 2):.0f} / {med(3, 2):.0f}; end {med(0, 5):.0f} / {med(3, 5):.0f}")
for h in range(min(4, (batch + 31) // 32)):
    a = [med(0, 16 + 4 * h + k) for k in range(4)]
    b = [med(3, 16 + 4 * h + k) for k in range(4)]
    print(f"  half-block {h}: GEMM start {a[0]:.0f}/{b[0]:.0f}  parked {a[1]:.0f}/{b[1]:.0f} (GEMM incl. the previous half-block's epilogue {a[1] - a[0]:.0f})  "
          f"past barrier {a[2]:.0f}/{b[2]:.0f} (wait {a[2] - a[1]:.0f})")
print(f"  last half-block finished by all eight waves: {med(0, 5) - med(0, 3):.0f} cycles")
if t[:, 0, 8].any():  # the 48 + 16 kernel of whole-mesh launches of 33..64 rows (flame_decode_head.hip) stamps its first MFMA
    print(f"  48 + 16: up-front basis requests issued {med(0, 16):.0f} / {med(3, 16):.0f}; first MFMA {med(0, 8):.0f} / {med(3, 8):.0f}; "
          f"pass 1 (rows 0..47) multiplied {med(0, 2):.0f} / {med(3, 2):.0f}, parked {med(0, 17):.0f} / {med(3, 17):.0f}; "
          f"pass 2 (rows 48..63) start {cyc(med(0, 20))} / {cyc(med(3, 20))}, parked {cyc(med(0, 21))} / {cyc(med(3, 21))}; "
          f"last barrier passed {med(0, 3):.0f} / {med(3, 3):.0f}")
    print(f"  48 + 16 stagers (wave 4): rows 48..63 requested {cyc(med(4, 16))}, written {cyc(med(4, 17))}; at barrier P1 {med(4, 18):.0f}, past it {med(4, 19):.0f}; "
          f"rows 32..47 finished {cyc(med(4, 21))}; past barrier P2 {cyc(med(4, 23))}")
    print(f"  48 + 16 stagers (wave 4 / 7): vertices 16..19 of rows 0..31 finished {cyc(med(4, 9))} / {cyc(med(7, 9))}")
    if batch > 48:  # the two seams (profiles/r12_kernel_log.md)
        print(f"  48 + 16 seams (mma wave 0): pass 1 multiplied -> chain start {cyc(med(0, 20) - med(0, 2))}; pass 1 parked (and announced) {cyc(med(0, 17))}, "
              f"`parked` seen / past P1 {cyc(med(0, 18))}; chain parked -> last barrier passed {cyc(med(0, 3) - med(0, 21))}; end {med(0, 5):.0f}")
print("stager waves (wave 4 / wave 7):")
print(f"  first loads issued {med(4, 1):.0f} / {med(7, 1):.0f}; past the first barrier {med(4, 6):.0f}; first part of A(0) published {med(4, 7):.0f}; "
      f"constants round 0 begun {cyc(med(4, 3))} / {cyc(med(7, 3))}, written {cyc(med(4, 4))} / {cyc(med(7, 4))}; A(0) published {med(4, 2):.0f}; end {med(4, 5):.0f}")
for h in range(min(4, (batch + 31) // 32)):
    a = [med(4, 16 + 4 * h + k) for k in range(4)]
    print(f"  phase {h}: start {a[0]:.0f}  A({h + 1}) written {a[1]:.0f}  loads issued {a[2]:.0f}  past barrier {a[3]:.0f}")
