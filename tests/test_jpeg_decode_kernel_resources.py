"""CPU: the four kernels of csrc/jpeg_decode.hip stay free of scratch and spills, and use the LDS DESIGN.md 4.19 states for each,
which is none: the scan compacts the restart markers with a ballot, an entropy lane keeps its bit reader in registers and its block in
global memory, the IDCT keeps its 64 values in registers, a pixel needs its neighbours' samples only. The registers bound the waves
per SIMD: 64 VGPRs (eight waves) for the scan, the entropy decode and the colour kernel, 168 (three waves) for the IDCT, whose lane
holds a whole block. Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

LDS_LIMIT = {"jpeg_scan_kernel": 0, "jpeg_entropy_kernel": 0, "jpeg_idct_kernel": 0, "jpeg_colour_kernel": 0}
VGPR_LIMIT = {"jpeg_scan_kernel": 64, "jpeg_entropy_kernel": 64, "jpeg_idct_kernel": 168, "jpeg_colour_kernel": 64}


@needs_hipcc
def test_jpeg_decode_no_scratch_no_spills_no_lds(tmp_path):
    kernels = resource_usage("jpeg_decode.hip", tmp_path)
    assert len(kernels) == 4, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= [v for key, v in VGPR_LIMIT.items() if key in name][0], (name, k)
