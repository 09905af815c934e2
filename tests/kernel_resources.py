"""Shared by the tests/test_*kernel_resources.py files: compile one unit of csrc for gfx950 with the flags csrc/Makefile builds
it with (hipcc cross-compiles without a GPU) and read back what the compiler says about its kernels. The command lines come
from a dry run of the Makefile's `all` target, so a flag that falls off a unit there falls off here too, and a unit that
leaves the object list has no command at all."""
import functools
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dad-3dheads_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@functools.lru_cache(maxsize=None)
def _build_commands():
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    argvs = [shlex.split(line) for line in out.stdout.splitlines() if " -c " in line]
    return {argv[argv.index("-c") + 1]: argv for argv in argvs}


def unit_command(source):
    """The argv `make all` compiles `source` with: [hipcc, flags.., -c, source, -o, object]."""
    commands = _build_commands()
    assert source in commands, f"{source} is not built by csrc/Makefile: {sorted(commands)}"
    return list(commands[source])


def _device_compile(source, mode, output):
    argv = unit_command(source)
    at = argv.index("-c")
    assert argv[at + 2] == "-o" and len(argv) == at + 4, argv
    out = subprocess.run([HIPCC, *argv[1:at], "--cuda-device-only", *mode, source, "-o", output], capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def device_assembly(source):
    """The gfx950 assembly text of the unit."""
    return _device_compile(source, ["-S"], "-").stdout


def resource_usage(source, tmp_path):
    """{kernel name: {field: value}} from the unit's `-Rpass-analysis=kernel-resource-usage` remarks."""
    out = _device_compile(source, ["-Rpass-analysis=kernel-resource-usage", "-c"], str(tmp_path / (source + ".o")))
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert kernels, "no kernel-resource-usage remarks: did the flag change?"
    return kernels
