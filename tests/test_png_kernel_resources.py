"""CPU: the three kernels of csrc/png_encode.hip stay free of scratch and spills, within the LDS DESIGN.md 4.15 states for each:
the filter a handful of reduction words, the segment deflate 56 KB (the segment, the parse's choice and jump tables, the visit
marks, the histograms, the tables and their work space; two workgroups per CU), the assemble one payload slot and its chunk
words. Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

SEGMENT = 8192
LDS_LIMIT = {"png_filter_kernel": 64, "deflate_segment_kernel": 56 * 1024, "png_assemble_kernel": SEGMENT + 16 + 12 + 32 + 64}


@needs_hipcc
def test_png_encode_no_scratch_no_spills_lds_within_the_budget(tmp_path):
    kernels = resource_usage("png_encode.hip", tmp_path)
    assert len(kernels) == 3, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # 256-thread workgroups, two per CU where the LDS allows it
