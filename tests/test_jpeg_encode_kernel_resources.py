"""CPU: the two kernels of csrc/jpeg_encode.hip stay free of scratch and spills, within the LDS and the registers DESIGN.md 4.20
states. jpeg_fdct_kernel holds a block's 64 samples in registers through both DCT passes and the quantiser, as the decoder's IDCT
does: 164 VGPRs, two waves per SIMD, no LDS. jpeg_pack_kernel keeps a chunk's bit image (54 032 bytes: 256 blocks at their worst),
one bit per byte of it for the restart markers, the two AC code tables and the words of its scans in LDS, 63 888 bytes, one
workgroup per CU, and 54 VGPRs.
Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

LDS_LIMIT = {"jpeg_fdct_kernel": 0, "jpeg_pack_kernel": 63888}
VGPR_LIMIT = {"jpeg_fdct_kernel": 168, "jpeg_pack_kernel": 64}


@needs_hipcc
def test_jpeg_encode_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("jpeg_encode.hip", tmp_path)
    assert len(kernels) == 2, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= [v for key, v in VGPR_LIMIT.items() if key in name][0], (name, k)
