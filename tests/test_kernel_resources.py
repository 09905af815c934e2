"""CPU: the kernels the metric rests on stay spill-free across compiler releases. Compiles the decode and Sim3DR translation units for
gfx950 with `-Rpass-analysis=kernel-resource-usage` (hipcc cross-compiles without a GPU) and asserts, for EVERY kernel in them: no scratch
(private segment 0 bytes per lane), no VGPR spills, and SGPR spills only where csrc documents them -- the pipelined decode kernel keeps
the exec mask of its role split in two lanes of a VGPR (one v_writelane pair at the top of the launch, one v_readlane pair at its end:
flame_decode_pipe.hip), the blend kernel of the alpha != 1 path its loop masks. The one exception is not on any BASELINE config: the
two-role kernel's FULL-POSE instantiations (K = 448: configs that drive neck and eyeballs, `flame_decode_kernel<28, false, ..>`) keep 20
bytes per lane on the stack. VERDICT r5 #5."""
import re

import pytest

from kernel_resources import device_assembly, needs_hipcc, resource_usage, unit_command

# (source, {kernel-name substring: SGPR spills allowed}, VGPR ceiling of the unit's hot kernel)
UNITS = [
    ("flame_decode_pipe.hip", {"flame_decode_pipe_kernel": 3}, 256),
    ("flame_decode_split.hip", {}, 256),
    ("flame_decode.hip", {"flame_decode_kernelILi26": 40, "flame_decode_kernelILi28": 96}, 256),  # (fallback + training forward; SCRATCH_OK below)
    ("sim3dr_kernels.hip", {"raster_blend_kernel": 24, "raster_kernel": 4, "tri_geometry_kernel": 8}, 128),
]
# units whose bit-exactness against the reference rests on unfused arithmetic, and why
NO_CONTRACTION = {
    "sim3dr_kernels.hip": "the reference extension is an SSE2 build without FMA: every multiply and add stays an individually rounded binary32 operation",
    "preprocess.hip": "the resize coefficients and the normalisation round each product and sum like the preprocessing oracle",
    "uv_texture.hip": "bit-equality with NumPy's float64 needs every product and sum rounded on its own",
    "train_objective.hip": "the reference's fp32 arithmetic has no FMAs (the floor-divide rule and the fp32 products of the landmark loss)",
    "train_batch.hip": "the barycentric products, the float64 scale-and-pad and the projection sums stay unfused",
}
SCRATCH_OK = {"flame_decode_kernelILi28ELb0": 32}  # bytes per lane: full-pose instantiations of the two-role kernel only


@needs_hipcc
@pytest.mark.parametrize("source,sgpr_ok,vgpr_cap", UNITS, ids=[u[0] for u in UNITS])
def test_no_scratch_no_vgpr_spills(source, sgpr_ok, vgpr_cap, tmp_path):
    kernels = resource_usage(source, tmp_path)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) <= max((n for key, n in SCRATCH_OK.items() if key in name), default=0), (name, k)
        assert int(k["VGPRs Spill"]) == 0, (name, k)
        allowed = max((n for key, n in sgpr_ok.items() if key in name), default=0)
        assert int(k["SGPRs Spill"]) <= allowed, (name, k, allowed)
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 256, (name, k)  # two waves per SIMD: 512 registers / 2
    hot = max(int(k["VGPRs"]) for k in kernels.values())
    assert hot <= vgpr_cap, (source, hot)
    print(source, {n[-60:]: (k["VGPRs"], k["SGPRs Spill"]) for n, k in kernels.items()})


@needs_hipcc
def test_split_kernels_register_budgets_and_no_packed_f32(tmp_path):
    """The fp16x2 form launches TEN waves per workgroup (three per SIMD on two of them): 512 / 3 -> at most 168 registers, without spills; the
    bf16x3 form eight (256). Neither may contain a packed-f32 VALU instruction: `v_pk_*_f32` in a wave beside a 16-bit MFMA stream returned wrong
    low halves (profiles/r06_kernel_log.md section 4) -- the file is built with -fno-slp-vectorize and scales its vectors element by element."""
    kernels = resource_usage("flame_decode_split.hip", tmp_path)
    f16 = {n: k for n, k in kernels.items() if "flame_decode_split_kernel" in n and "F16x2" in n}
    bf16 = {n: k for n, k in kernels.items() if "flame_decode_split_kernel" in n and "Bf16x3" in n}
    assert len(f16) == 4 and len(bf16) == 4, list(kernels)  # TO2D x write-back / write-through stores
    for name, k in f16.items():
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 168 and int(k["Occupancy"]) >= 3, (name, k)
    for name, k in bf16.items():
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 256 and int(k["Occupancy"]) >= 2, (name, k)
    assert "-fno-slp-vectorize" in unit_command("flame_decode_split.hip")
    asm = device_assembly("flame_decode_split.hip")
    packed = sorted(set(re.findall(r"\bv_pk_\w*f32\b", asm)))
    assert not packed, packed
    assert asm.count("v_mfma_f32_16x16x32_f16") > 0 and asm.count("v_mfma_f32_16x16x32_bf16") > 0


@pytest.mark.parametrize("source", NO_CONTRACTION)
def test_unit_is_built_without_contraction(source):
    assert "-ffp-contract=off" in unit_command(source), NO_CONTRACTION[source]
