"""CPU: the kernels of csrc/preprocess_boxes.hip stay free of scratch and spills. Compiled for gfx950 with the flags of
csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_preprocess_boxes_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("preprocess_boxes.hip", tmp_path)
    boxes = [n for n in kernels if "preprocess_boxes_kernel" in n]
    params = [n for n in kernels if "readjust_frame_kernel" in n and "points" not in n]
    points = [n for n in kernels if "points_readjust_frame_kernel" in n]
    # one preprocess kernel per output format (float32 planar, fp16 and bf16 channels-last); the box dtype is a run-time switch
    assert len(boxes) == 3 and len(params) == 1 and len(points) == 1 and len(kernels) == 5, sorted(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) == 0, (name, k)  # a streaming kernel: nothing is shared between lanes but one shuffle
    # 256-thread workgroups of a memory-bound kernel: eight waves a SIMD need <= 64 registers a lane
    for name in boxes:
        assert int(kernels[name]["VGPRs"]) <= 64, (name, kernels[name])


@needs_hipcc
def test_preprocess_boxes_is_built_without_fp_contraction():
    """extend_bbox's `x - w * left` and the normalisation's `(v - mean) * inv` round each product and sum on their own, as numpy does."""
    assert "-ffp-contract=off" in unit_command("preprocess_boxes.hip")
