"""CPU: the training-batch keypoint kernel (csrc/train_batch.hip) has no scratch and no spills. Compiled for gfx950 with the
flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
import os

from kernel_resources import CSRC, needs_hipcc, resource_usage


@needs_hipcc
def test_train_batch_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("train_batch.hip", tmp_path)
    assert len(kernels) == 1 and "gt_keypoints_kernel" in next(iter(kernels)), list(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) == 0, (name, k)
        assert int(k["VGPRs"]) <= 64, (name, k)


def test_projection_arithmetic_has_one_copy():
    """project_vertices_kernel and the training-batch kernel share projection_math.hpp; neither restates the sums."""
    for fn in ("projection.hip", "train_batch.hip"):
        src = open(os.path.join(CSRC, fn)).read()
        assert '#include "projection_math.hpp"' in src, fn
        assert "mv[4 * i]" not in src and "pm[4 * i]" not in src, fn
