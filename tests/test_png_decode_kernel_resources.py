"""CPU: the six kernels of csrc/png_decode.hip stay free of scratch and spills, within the LDS DESIGN.md 4.16 states for each: the
scan and the unfilter none (registers and shuffles), a segment's inflate and its second pass 20 KB (a 16 KB window, 2 KB of staged input, the tables:
eight one-wave workgroups per CU), the whole-stream inflate 36 KB (the 32 KB window of deflate: four per CU). Compiled for gfx950
with the flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage

LDS_LIMIT = {"png_scan_kernel": 0, "png_segment_kernel": 20 * 1024, "png_segment_fix_kernel": 20 * 1024, "png_inflate_kernel": 36 * 1024, "zlib_inflate_kernel": 36 * 1024,
             "png_unfilter_kernel": 0}


@needs_hipcc
def test_png_decode_no_scratch_no_spills_lds_within_the_budget(tmp_path):
    kernels = resource_usage("png_decode.hip", tmp_path)
    assert len(kernels) == 6, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # one-wave workgroups: the LDS, not the registers, bounds the waves per CU
