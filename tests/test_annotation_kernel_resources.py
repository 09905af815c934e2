"""CPU: the kernel of csrc/annotation_parse.hip stays free of scratch and spills and within the registers and LDS DESIGN.md 4.18 states:
one 256-lane workgroup per document, a lane's 16 bytes held in four registers and picked apart with selects, and 34 KiB of LDS or less:
the tile's token kinds (4 098 bytes), its key records (1 367 x 21 bytes: record, name, hash), the hashes of the document's 128 keys, the
output pointers and the reduction words. That LDS lets four workgroups share a CU (160 KiB / 34 KiB), four waves per SIMD, so the kernel
stays at 128 VGPRs or fewer (512 / 128 = 4 waves): registers never hold fewer workgroups than the LDS does.
Compiled for gfx950 with the flags of csrc/Makefile (tests/kernel_resources.py); only the compiler's resource remarks are read."""
from kernel_resources import needs_hipcc, resource_usage


@needs_hipcc
def test_annotation_parse_no_scratch_no_spills_bounded_lds(tmp_path):
    kernels = resource_usage("annotation_parse.hip", tmp_path)
    assert len(kernels) == 1, list(kernels)
    for name, k in kernels.items():
        assert "annotation_parse_kernel" in name
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 34 * 1024, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)
