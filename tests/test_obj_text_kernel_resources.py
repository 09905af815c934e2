"""CPU: the two kernels of csrc/obj_text.hip stay free of scratch and spills, within the LDS their tile states in DESIGN.md 4.12
(a tile of 256 lines: 18 192 bytes of text image + 3 072 bytes of coordinates + the reduction words), and the text leaves the
write kernel in 16-byte stores. Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py)."""
from kernel_resources import device_assembly, needs_hipcc, resource_usage

TILE_LINES, MAX_LINE = 256, 71
STAGE_BYTES = (TILE_LINES * MAX_LINE + 15 + 15) // 16 * 16
LDS_LIMIT = {"obj_line_lengths_kernel": TILE_LINES * 12 + 512, "obj_write_text_kernel": STAGE_BYTES + TILE_LINES * 12 + 512}


@needs_hipcc
def test_obj_text_no_scratch_no_spills_lds_within_the_tile(tmp_path):
    kernels = resource_usage("obj_text.hip", tmp_path)
    assert len(kernels) == 2, list(kernels)
    for name, k in kernels.items():
        limit = [v for key, v in LDS_LIMIT.items() if key in name]
        assert len(limit) == 1, name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= limit[0], (name, k)
        assert int(k["VGPRs"]) <= 64, (name, k)  # 256-thread workgroups, 8 waves per SIMD


@needs_hipcc
def test_obj_text_leaves_in_wide_stores():
    asm = device_assembly("obj_text.hip")
    body = asm[asm.index("obj_write_text_kernel"):]
    assert "global_store_dwordx4" in body and ("ds_read_b128" in body or "ds_read2_b64" in body)
    assert "scratch_" not in asm
