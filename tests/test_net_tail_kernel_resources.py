"""CPU: the kernels of csrc/net_tail.hip stay free of scratch and vector-register spills and within the LDS DESIGN.md 4.31 states (the
pooling slices: 8 KB; a layer workgroup's staged tile of 16 images: 32 KB), and the unit is built without floating-point contraction.
Compiled for gfx950 with the flags of csrc/Makefile and `-Rpass-analysis=kernel-resource-usage` (tests/kernel_resources.py)."""
from kernel_resources import needs_hipcc, resource_usage, unit_command


@needs_hipcc
def test_net_tail_kernels_no_scratch_no_vgpr_spills_bounded_lds(tmp_path):
    kernels = resource_usage("net_tail.hip", tmp_path)
    lds_limit = {"nhwc_fusion_concat_kernel": 0, "nhwc_bias_mul_kernel": 0, "heads_pool_kernel": 8192, "heads_layer_kernel": 32768}
    assert len(kernels) == 3 * 2 + 3 + 3 * 2, list(kernels)  # three dtypes; the layer kernel with one and with four rows per wave
    for name, k in kernels.items():
        key = [key for key in lds_limit if key in name]
        assert len(key) == 1, name
        assert int(k["ScratchSize"]) == 0 and int(k["VGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= lds_limit[key[0]], (name, k)
        assert int(k["VGPRs"]) <= 256, (name, k)  # two waves per SIMD at least


@needs_hipcc
def test_net_tail_unit_is_built_without_contraction():
    """The interpolation, the add-then-multiply and the activations are stated operation by operation; only fmaf() fuses."""
    assert "-ffp-contract=off" in unit_command("net_tail.hip")
