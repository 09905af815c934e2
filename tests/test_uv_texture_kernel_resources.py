"""CPU: the UV-texture kernels (csrc/uv_texture.hip) stay free of scratch and spills, within 64 KB of LDS. Compiled for gfx950
with the flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage


@needs_hipcc
def test_uv_texture_no_scratch_no_spills(tmp_path):
    kernels = resource_usage("uv_texture.hip", tmp_path)
    assert sorted(n for n in kernels if "vertex_normals_kernel" in n or "bake_kernel" in n) == sorted(kernels), list(kernels)
    assert len(kernels) == 2, list(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # 256-thread workgroups, at least 4 waves per SIMD
