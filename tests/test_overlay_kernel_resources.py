"""CPU: the two kernels of csrc/overlay.hip stay free of scratch and spills: a lane's pixels live in registers from the one load to
the one store, and the chunk's in-order list is the only LDS. Compiled for gfx950 with the flags of csrc/Makefile
(tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage


@needs_hipcc
def test_overlay_two_kernels_no_scratch_no_spills_lds_within_64_kb(tmp_path):
    kernels = resource_usage("overlay.hip", tmp_path)
    assert len(kernels) == 2, list(kernels)
    assert sorted(sum(key in name for name in kernels) for key in ("overlay_segments_kernel", "overlay_discs_kernel")) == [1, 1]
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
