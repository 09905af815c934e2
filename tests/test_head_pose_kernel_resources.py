"""CPU: the two kernels of csrc/head_pose.hip stay free of scratch and spills: the 3x3 Jacobi SVD of csrc/pose_math.hpp indexes no
array by a run-time value, so a row's (or an item's) whole state lives in registers. Compiled for gfx950 with the
flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_head_pose_two_kernels_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("head_pose.hip", tmp_path)
    assert len(kernels) == 2, list(kernels)
    assert sorted(sum(key in name for name in kernels) for key in ("head_pose_kernel", "procrustes_kernel")) == [1, 1]
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) == 0, (name, k)


@needs_hipcc
def test_head_pose_unit_is_built_without_contraction():
    """The host entries and the kernels round the same operations only while neither fuses a product into a sum."""
    assert "-ffp-contract=off" in unit_command("head_pose.hip")
