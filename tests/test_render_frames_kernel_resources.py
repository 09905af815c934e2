"""CPU: the kernels of csrc/sim3dr_frames.hip stay free of scratch and spills, and the unit keeps the reference's unfused arithmetic.
Compiled for gfx950 with the flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_frames_kernels_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("sim3dr_frames.hip", tmp_path)
    want = ("frames_setup_kernel", "frames_box_kernel", "frames_plan_kernel", "frames_bin_kernel", "frames_scan_kernel", "frames_tile_kernel")
    for stem in want:
        assert any(stem in n for n in kernels), (stem, sorted(kernels))
    assert len(kernels) == 7, sorted(kernels)  # frames_bin_kernel twice: count and fill
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
    tile = next(k for n, k in kernels.items() if "frames_tile_kernel" in n)
    assert int(tile["LDS Size"]) == 64 * 64 * 8, tile  # the keys of one tile and nothing else: five workgroups a CU
    assert int(tile["VGPRs"]) <= 128, tile             # 256 threads: two waves a SIMD per workgroup at any count up to 256; <= 128 keeps four


@needs_hipcc
def test_frames_unit_is_built_without_fp_contraction():
    """The pixel test, the depth and the colour are sums of products the reference rounds one by one (an SSE2 build without FMA)."""
    assert "-ffp-contract=off" in unit_command("sim3dr_frames.hip")
