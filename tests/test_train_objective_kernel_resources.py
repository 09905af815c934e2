"""CPU: the training-objective kernels (csrc/train_objective.hip) stay free of scratch and spills, within 64 KB of LDS. Compiled
for gfx950 with the flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

KERNELS = ("heatmap_encode_kernel", "iou_terms_kernel", "iou_finish_kernel", "iou_grad_kernel", "visibility_loss_kernel",
           "keypoint_err_kernel", "keypoint_finish_kernel")


@needs_hipcc
def test_train_objective_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("train_objective.hip", tmp_path)
    assert all(any(k in n for k in KERNELS) for n in kernels), list(kernels)
    assert all(any(k in n for n in kernels) for k in KERNELS), list(kernels)
    assert len(kernels) == 2 + 8 + 1 + 4 + 1 + 2 + 1, list(kernels)  # template instances
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)
