"""CPU: the one kernel of csrc/track_assign.hip stays free of scratch and spills, its LDS is the sum its header states, and the unit
is built without floating-point contraction. Compiled for gfx950 with the flags of csrc/Makefile and
`-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
import os
import re

from kernel_resources import ROOT, needs_hipcc, resource_usage, unit_command

from dad_3dheads_amd import _lib


@needs_hipcc
def test_track_assign_one_kernel_no_scratch_no_spills_and_the_stated_lds(tmp_path):
    kernels = resource_usage("track_assign.hip", tmp_path)
    assert len(kernels) == 1 and "assign_detections_kernel" in next(iter(kernels)), sorted(kernels)  # one launch, one kernel
    k = next(iter(kernels.values()))
    assert int(k["ScratchSize"]) == 0, k
    assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, k
    slots, dets = _lib.TRACK_MAX_SLOTS, _lib.TRACK_MAX_DETECTIONS
    # the pass bits (a bit per pair), the staged slot boxes (16 bytes) and frames (4 bytes), two lists of one int per lane, the two free
    # masks (a bit per slot, a bit per detection), the scans' word per wave and the rounds' two words
    stated = dets * slots // 8 + slots * 16 + slots * 4 + 2 * 1024 * 4 + slots // 8 + dets // 8 + (1024 // 64) * 4 + 2 * 4
    assert int(k["LDS Size"]) == stated == 160072, k
    assert int(k["LDS Size"]) <= 160 * 1024  # one CU's LDS on gfx950
    assert int(k["VGPRs"]) <= 128, k  # one workgroup of 1024 lanes: four waves a SIMD
    for text in (open(os.path.join(ROOT, "include", "dad3d.h")).read(), open(os.path.join(ROOT, "dad-3dheads_amd", "csrc", "track_assign.hip")).read()):
        assert re.search(r"160 072 bytes", text)  # the header and the unit state the same sum


@needs_hipcc
def test_track_assign_is_built_without_fp_contraction():
    """`match_iou * double(union)` is one rounded product, as the numpy statement of the rule computes it."""
    assert "-ffp-contract=off" in unit_command("track_assign.hip")
