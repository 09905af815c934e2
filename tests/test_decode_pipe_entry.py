"""CPU: the pipelined decode kernel's arguments arrive with the wave. Compiles flame_decode_pipe.hip for gfx950 with the flags csrc/Makefile
gives the unit (hipcc cross-compiles without a GPU) and holds, for all three instantiations, the kernel descriptor and the code-object
metadata to the argument list in the source: the number of preloaded kernarg dwords is the constant written next to that list, every argument
the code in front of the start-up barrier reads lies inside the preloaded range, the by-value struct of the remaining arguments starts exactly
where the range ends (the kernel reads it through the kernarg pointer at that offset), and the register budget of
tests/test_kernel_resources.py holds."""
import os
import re

from kernel_resources import CSRC, device_assembly, needs_hipcc, resource_usage, unit_command

SOURCE = "flame_decode_pipe.hip"
INSTANTIATIONS = ("ILb1ELb0E", "ILb0ELb0E", "ILb1ELb1E")  # <TO2D, CHUNKED>: 2-D, 3-component projection, chunked landmark sub-model
# what the code in front of the start-up barrier reads, under the kernel's parameter names: the rows and their geometry, the vertex table, the
# basis pack, the trace pointer, and the word that carries the flags (and a chunked launch's geometry: `span_half` is its chunk_half)
PRE_BARRIER = ("params", "n_params", "batch", "span_half", "n_verts", "vtab", "bpack", "trace_buf", "geom")
SGPR_SPILLS_ALLOWED = 3  # tests/test_kernel_resources.py, UNITS


def _source():
    with open(os.path.join(CSRC, SOURCE)) as f:
        return f.read()


def _parameter_names(src):
    m = re.search(r"void flame_decode_pipe_kernel\((.*?)\)\s*\{", src, re.S)
    assert m, "kernel signature not found"
    names = [re.search(r"(\w+)\s*$", p.strip()).group(1) for p in m.group(1).split(",")]
    assert len(set(names)) == len(names), names
    return names


def _kernels(asm):
    """{mangled name: (preload length from the descriptor, [(offset, size) of every explicit argument])}"""
    descr = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", asm, re.S)}
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        args_text = block[block.index(".args:"):block.index(".group_segment_fixed_size")]
        args = [(int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)", args_text)]
        out[name] = (descr[name], args)
    return out


@needs_hipcc
def test_arguments_are_preloaded_and_the_pre_barrier_set_lies_inside(tmp_path):
    src = _source()
    m = re.search(r"constexpr int kPipePreloadDwords = (\d+);", src)
    assert m, "the constant next to the argument list"
    preload = int(m.group(1))
    assert preload > 0
    assert f"-amdgpu-kernarg-preload-count={preload}" in unit_command(SOURCE), "the Makefile asks for what the source counts on"
    names = _parameter_names(src)
    assert set(PRE_BARRIER) <= set(names), names
    kernels = {n: k for n, k in _kernels(device_assembly(SOURCE)).items() if "flame_decode_pipe_kernel" in n}
    assert len(kernels) == 3 and all(any(i in n for n in kernels) for i in INSTANTIATIONS), list(kernels)
    for name, (length, args) in kernels.items():
        assert length == preload, (name, length)
        assert len(args) == len(names), (name, args, names)  # explicit arguments only: the kernel reads no hidden ones
        at = dict(zip(names, args))
        for arg in PRE_BARRIER:
            offset, size = at[arg]
            assert offset + size <= 4 * preload, (name, arg, offset, size)
        # the struct behind the range: the kernel reads it at kernarg + 4 * kPipePreloadDwords
        assert names[-1] == "late" and at["late"][0] == 4 * preload, (name, at["late"])
        # nothing between the arguments: the range is full of arguments, not padding
        assert [o for o, _ in args] == [sum(s for _, s in args[:i]) for i in range(len(args))], (name, args)
    usage = {n: k for n, k in resource_usage(SOURCE, tmp_path).items() if "flame_decode_pipe_kernel" in n}
    assert len(usage) == 3, list(usage)
    for name, k in usage.items():
        assert int(k["ScratchSize"]) == 0 and int(k["VGPRs Spill"]) == 0, (name, k)
        assert int(k["SGPRs Spill"]) <= SGPR_SPILLS_ALLOWED, (name, k)
        assert int(k["VGPRs"]) + int(k.get("AGPRs", 0)) <= 256, (name, k)
