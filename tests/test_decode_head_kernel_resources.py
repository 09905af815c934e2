"""CPU: the register and argument bounds of the decode kernel for whole-mesh launches of 33..64 rows (flame_decode_head.hip). Compiles the unit
for gfx950 with the flags csrc/Makefile gives it (hipcc cross-compiles without a GPU) and holds both instantiations to: no scratch, no VGPR
spills, VGPRs + AGPRs <= 256 (two waves per SIMD), at most three SGPR spills -- and those only the exec-mask pair of the role split, written
to VGPR lanes once and read back once, never inside a loop or to scratch --, and fourteen kernarg dwords preloaded, the struct of the late
arguments starting where that range ends."""
import re

from kernel_resources import device_assembly, needs_hipcc, resource_usage, unit_command

SOURCE = "flame_decode_head.hip"
KERNEL = "flame_decode_head_kernel"
INSTANTIATIONS = ("ILb1EE", "ILb0EE")  # <TO2D>
PRELOAD = 14
SGPR_SPILLS_ALLOWED = 3


@needs_hipcc
def test_head_kernel_register_bounds(tmp_path):
    usage = {n: k for n, k in resource_usage(SOURCE, tmp_path).items() if KERNEL in n}
    assert len(usage) == 2 and all(any(i in n for n in usage) for i in INSTANTIATIONS), list(usage)
    assert not any("flame_decode_pipe_kernel" in n for n in usage)
    for name, k in usage.items():
        print(name, k)
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0, (name, k)
        assert int(k["SGPRs Spill"]) <= SGPR_SPILLS_ALLOWED, (name, k)
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 256, (name, k)
        assert int(k["Occupancy"]) >= 2, (name, k)


@needs_hipcc
def test_head_kernel_sgpr_spills_are_the_role_split_pair():
    """An SGPR spill of this kernel is a v_writelane_b32 into a VGPR lane and a v_readlane_b32 back. The documented ones save the exec mask of the
    stager / mma role split: one 64-bit pair, so at most two lanes written per kernel besides a third the budget allows, every lane written once
    (no spill inside an unrolled loop body) and nothing spilled to scratch memory."""
    asm = device_assembly(SOURCE)
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"\n(_Z\w*" + KERNEL + r"\w*):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", asm, re.S)}
    assert len(bodies) == 2, list(bodies)
    for name, body in bodies.items():
        writes = re.findall(r"v_writelane_b32 (v\d+), (\S+), (\d+)", body)
        lanes = [(reg, lane) for reg, _, lane in writes]
        assert len(lanes) <= SGPR_SPILLS_ALLOWED, (name, writes)
        assert len(set(lanes)) == len(lanes), (name, writes)
        assert not re.search(r"\bscratch_(load|store)|\bbuffer_(load|store)\w* .*offen.*; \d+-byte Folded (Spill|Reload)", body), name


@needs_hipcc
def test_head_kernel_arguments_are_preloaded():
    assert f"-amdgpu-kernarg-preload-count={PRELOAD}" in unit_command(SOURCE)
    assert unit_command(SOURCE)[1:-4] == unit_command("flame_decode_pipe.hip")[1:-4], "the unit is built as the pipelined unit is"
    asm = device_assembly(SOURCE)
    descr = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", asm, re.S)}
    descr = {n: v for n, v in descr.items() if KERNEL in n}
    assert len(descr) == 2 and all(v == PRELOAD for v in descr.values()), descr
    meta = asm[asm.index("amdhsa.kernels:"):]
    seen = 0
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if KERNEL not in name:
            continue
        seen += 1
        args_text = block[block.index(".args:"):block.index(".group_segment_fixed_size")]
        args = [(int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)", args_text)]
        assert len(args) == 11, (name, args)  # explicit arguments only: ten preloaded scalars and the struct behind them
        assert [o for o, _ in args] == [sum(s for _, s in args[:i]) for i in range(len(args))], (name, args)  # no padding
        assert args[-1][0] == 4 * PRELOAD, (name, args)  # late_args() reads the struct at kernarg + 4 * 14
    assert seen == 2
