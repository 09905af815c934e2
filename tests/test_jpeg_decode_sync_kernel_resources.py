"""CPU: the five kernels of csrc/jpeg_decode_sync.hip stay free of scratch and spills, and within the LDS and the registers
DESIGN.md 4.21 states: the groups kernel holds the file's six Huffman tables (924 bytes each), the 256 states of its pieces and the
words of its collectives in LDS, the write kernel the tables alone, the totals kernel its collectives' words; a piece keeps its bit
reader and its state in registers, at most 64 VGPRs, so eight waves fit a SIMD. Compiled for gfx950 with the flags of csrc/Makefile
(tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

LDS_LIMIT = {"jpeg_sync_clear_kernel": 0, "jpeg_sync_segments_kernel": 0, "jpeg_sync_groups_kernel": 8192, "jpeg_sync_totals_kernel": 512,
             "jpeg_sync_write_kernel": 6 * 924}
VGPR_LIMIT = 64


@needs_hipcc
def test_jpeg_decode_sync_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("jpeg_decode_sync.hip", tmp_path)
    assert len(kernels) == 5, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= VGPR_LIMIT, (name, k)
