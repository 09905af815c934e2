"""CPU: the kernel of csrc/track_boxes.hip stays free of scratch and spills. Compiled for gfx950 with the flags of csrc/Makefile
and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import device_assembly, needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_track_boxes_one_kernel_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("track_boxes.hip", tmp_path)
    assert len(kernels) == 1 and "boxes_from_heads_kernel" in next(iter(kernels)), sorted(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) == 4 * 5 * 4, (name, k)  # the reduction's record of five words, one per wave, and nothing else
        assert int(k["VGPRs"]) <= 64, (name, k)  # 256-thread workgroups of a memory-bound kernel: eight waves a SIMD


@needs_hipcc
def test_track_boxes_has_no_atomics():
    """Every head is one workgroup's: nothing is combined through memory."""
    text = device_assembly("track_boxes.hip")
    assert "boxes_from_heads_kernel" in text
    assert "atomic" not in text.lower()


@needs_hipcc
def test_track_boxes_is_built_without_fp_contraction():
    """`min_visible * double(w * h)` is one rounded product, as the host statement of the rule computes it."""
    assert "-ffp-contract=off" in unit_command("track_boxes.hip")
