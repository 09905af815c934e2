"""CPU: the two kernels of csrc/json_text.hip stay free of scratch and spills, at 64 VGPRs or fewer, and within the LDS their tile
states in DESIGN.md 4.13: a tile of 256 slots, each up to a literal at the cap (64 bytes) and the longest number (23 bytes), the
suffix (64 bytes) and up to 15 bytes of lead-in on either end -- 22 352 bytes of text image in the write kernel, plus the
reduction words. The length kernel stages nothing. Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py);
only the compiler's resource remarks are read."""
from kernel_resources import needs_hipcc, resource_usage

TILE_SLOTS, MAX_LITERAL, MAX_NUMBER = 256, 64, 23
STAGE_BYTES = (TILE_SLOTS * (MAX_LITERAL + MAX_NUMBER) + MAX_LITERAL + 15 + 15) // 16 * 16
LDS_LIMIT = {"json_slot_lengths_kernel": 512, "json_write_text_kernel": STAGE_BYTES + 512}


@needs_hipcc
def test_json_text_no_scratch_no_spills_lds_within_the_tile(tmp_path):
    assert STAGE_BYTES == 22352
    kernels = resource_usage("json_text.hip", tmp_path)
    assert len(kernels) == 2, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= 64, (name, k)  # 256-thread workgroups, 8 waves per SIMD
