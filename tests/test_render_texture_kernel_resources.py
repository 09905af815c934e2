"""CPU: the tile kernel of the textured render (`render_texture_kernel`, csrc/sim3dr_kernels.hip) stays free of scratch and
spills within 128 VGPRs (two 512-thread workgroups per CU), in a unit built without contraction. Compiled for gfx950 with the
flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import device_assembly, needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_render_texture_kernel_no_scratch_no_spills(tmp_path):
    kernels = {n: k for n, k in resource_usage("sim3dr_kernels.hip", tmp_path).items() if "render_texture_kernel" in n}
    assert len(kernels) == 4, list(kernels)  # float / uint8 image x float / uint8 texture
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 128, (name, k)
        assert int(k["LDS Size"]) <= 40 * 1024, (name, k)  # the 64x64 keys: at least two workgroups per CU beside other kernels
    assert "-ffp-contract=off" in unit_command("sim3dr_kernels.hip")


@needs_hipcc
def test_render_texture_kernel_has_no_fused_multiply_add():
    """Bit-equality with the reference's SSE2 arithmetic: no v_fma / v_mac / v_fmac on f32 anywhere in the kernel's bodies."""
    asm = device_assembly("sim3dr_kernels.hip")
    bodies = [part.split(".end_amdhsa_kernel")[0] for part in asm.split(".globl")[1:] if "render_texture_kernel" in part.split("\n", 1)[0]]
    assert len(bodies) >= 4
    for body in bodies:
        code = body.split("s_endpgm")[0]
        assert "ds_max_u64" in code or "ds_max_rtn_u64" in code  # the LDS z-buffer
        for op in ("v_fma_f32", "v_fmac_f32", "v_mac_f32", "v_mad_f32", "v_pk_fma_f32"):
            assert op not in code, op
