"""CPU: the two kernels of csrc/track_steady.hip stay free of scratch and spills, the unit is built without floating-point
contraction, and the LDS of the duplicate kernel is what its design states. Compiled for gfx950 with the flags of csrc/Makefile
and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command

from dad_3dheads_amd import _lib


@needs_hipcc
def test_track_steady_two_kernels_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("track_steady.hip", tmp_path)
    assert len(kernels) == 2, sorted(kernels)
    euro = next(k for name, k in kernels.items() if "one_euro_rows_kernel" in name)
    dup = next(k for name, k in kernels.items() if "suppress_duplicates_kernel" in name)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
    assert int(euro["LDS Size"]) == 0, euro  # a wave a row: the only collective is a wave reduction
    assert int(euro["VGPRs"]) <= 64, euro  # 256-thread workgroups of a memory-bound kernel: eight waves a SIMD
    # the pair bits of all slots (n^2 / 8 bytes at the cap), the staged boxes (16 bytes a slot) and frame numbers (4 bytes a slot)
    cap = _lib.TRACK_MAX_SLOTS
    assert int(dup["LDS Size"]) == cap * cap // 8 + cap * 16 + cap * 4 == 151552, dup
    assert int(dup["LDS Size"]) <= 160 * 1024  # one CU's LDS on gfx950
    assert int(dup["VGPRs"]) <= 128, dup  # one workgroup of 1024 lanes: four waves a SIMD


@needs_hipcc
def test_track_steady_is_built_without_fp_contraction():
    """Every operation of the filter rounds once, as the numpy statement of the rule computes it; `merge_iou * double(union)` is
    one rounded product."""
    assert "-ffp-contract=off" in unit_command("track_steady.hip")
