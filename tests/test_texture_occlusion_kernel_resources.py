"""CPU: the kernels of csrc/uv_texture_occlusion.hip (the depth maps of heads in frames and the bake with the depth test) stay free of
scratch and spills and within 128 VGPRs, and the unit keeps the references' unfused arithmetic. Compiled for gfx950 with the flags of
csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command

UNIT = "uv_texture_occlusion.hip"
KERNELS = ("depth_window_kernel", "depth_clear_kernel", "depth_raster_kernel", "bake_frames_occluded_kernel")


@needs_hipcc
def test_occlusion_kernels_no_scratch_no_spills_128_vgprs(tmp_path):
    kernels = resource_usage(UNIT, tmp_path)
    assert len(kernels) == len(KERNELS) and all(any(k in name for name in kernels) for k in KERNELS), sorted(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # 256-thread workgroups, at least 4 waves per SIMD
        if "depth_window_kernel" not in name:
            assert int(k["LDS Size"]) == 0, (name, k)  # only the window reduction keeps its partial results in LDS


@needs_hipcc
def test_unit_is_built_without_fp_contraction():
    """The depth is the reference's w0 * z0 + w1 * z1 + w2 * z2 and the depth test NumPy's float64 sums of products, rounded one by one."""
    assert "-ffp-contract=off" in unit_command(UNIT)


@needs_hipcc
def test_the_bake_from_frames_keeps_its_one_kernel(tmp_path):
    """The depth test lives in a unit of its own: uv_texture_frames.hip still holds bake_frames_kernel and nothing else."""
    kernels = resource_usage("uv_texture_frames.hip", tmp_path)
    assert len(kernels) == 1 and all("bake_frames_kernel" in n for n in kernels), sorted(kernels)
