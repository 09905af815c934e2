"""CPU: the kernels of csrc/uv_texture_frames.hip and csrc/sim3dr_frames_texture.hip stay free of scratch and spills, the textured tile
kernel keeps the frames chain's occupancy, and both units keep the reference's unfused arithmetic. Compiled for gfx950 with the flags
of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
import pytest

from kernel_resources import needs_hipcc, resource_usage, unit_command


def _clean(kernels):
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)


@needs_hipcc
def test_bake_frames_kernel_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("uv_texture_frames.hip", tmp_path)
    assert len(kernels) == 1 and all("bake_frames_kernel" in n for n in kernels), sorted(kernels)
    _clean(kernels)
    for name, k in kernels.items():
        assert int(k["LDS Size"]) == 0, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # 256-thread workgroups, at least 4 waves per SIMD


@needs_hipcc
def test_textured_tile_kernel_no_scratch_no_spills_five_workgroups_a_cu(tmp_path):
    kernels = resource_usage("sim3dr_frames_texture.hip", tmp_path)
    assert len(kernels) == 2 and all("frames_texture_tile_kernel" in n for n in kernels), sorted(kernels)  # uint8 and float32 textures
    _clean(kernels)
    for name, k in kernels.items():
        assert int(k["LDS Size"]) == 64 * 64 * 8, (name, k)  # the keys of one tile and nothing else: five workgroups a CU
        assert int(k["VGPRs"]) <= 128, (name, k)


@needs_hipcc
@pytest.mark.parametrize("unit", ["uv_texture_frames.hip", "sim3dr_frames_texture.hip"])
def test_units_are_built_without_fp_contraction(unit):
    """The candidate's point and normal, the pixel test, the depth and the texel are sums of products the references round one by one."""
    assert "-ffp-contract=off" in unit_command(unit)
