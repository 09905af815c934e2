"""CPU: the kernels of csrc/heatmap_points.hip stay free of scratch and spills. Compiled for gfx950 with the flags of
csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage


@needs_hipcc
def test_heatmap_points_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("heatmap_points.hip", tmp_path)
    nchw = [n for n in kernels if "heatmap_argmax_nchw_kernel" in n]
    nhwc = [n for n in kernels if "heatmap_argmax_nhwc_kernel" in n]
    unpack = [n for n in kernels if "heatmap_argmax_unpack_kernel" in n]
    pts = [n for n in kernels if "points_readjust_kernel" in n]
    # four dtypes; per dtype one channels-last kernel for every load width from one element to 16 bytes: 3 + 4 + 4 + 5
    assert len(nchw) == 4 and len(nhwc) == 16 and len(unpack) == 4 and len(pts) == 1, sorted(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
    # 512-thread workgroups, eight waves on four SIMDs: two workgroups per CU need <= 128 registers a lane
    for name in nhwc:
        assert int(kernels[name]["VGPRs"]) <= 128, (name, kernels[name])
