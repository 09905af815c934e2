"""CPU: the benchmark scorer's kernels (csrc/mesh_eval.hip) stay free of scratch and spills. Compiled for gfx950 with the flags of
csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage


@needs_hipcc
def test_mesh_eval_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("mesh_eval.hip", tmp_path)
    nn = [n for n in kernels if "nearest_kernel" in n]
    z5 = [n for n in kernels if "z5_rank_kernel" in n]
    assert len(nn) == 8 and len(z5) == 1, list(kernels)  # k = 1..8
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
    # 1024-thread sort workgroups: 16 waves on 4 SIMDs need <= 128 registers each
    assert int(kernels[z5[0]]["VGPRs"]) <= 128, kernels[z5[0]]
