"""CPU: the six kernels of csrc/json_parse.hip stay free of scratch and spills and within the registers and LDS DESIGN.md 4.14 states:
256-lane workgroups at 64 VGPRs or fewer (8 waves per SIMD), a lane's 16 bytes held in four registers and picked apart with selects (no
indexing into memory), and no LDS but the reduction words (16 bytes; the array check's workgroup vote may take up to 512). Compiled for
gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py); only the compiler's resource remarks are read."""
from kernel_resources import needs_hipcc, resource_usage

LDS_LIMIT = {"json_tile_quotes_kernel": 16, "json_scan_tiles_kernel": 16, "json_classify_kernel": 16, "json_compact_kernel": 16,
             "json_check_arrays_kernel": 512, "json_values_kernel": 0}


@needs_hipcc
def test_json_parse_no_scratch_no_spills_small_lds(tmp_path):
    kernels = resource_usage("json_parse.hip", tmp_path)
    assert len(kernels) == 6, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= 64, (name, k)
