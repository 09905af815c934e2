"""CPU: the UV-texture kernels (csrc/uv_texture.hip) stay free of scratch and spills, within 64 KB of LDS. Compiled for gfx950
with `-Rpass-analysis=kernel-resource-usage` and the Makefile's -ffp-contract=off, as in tests/test_eval_kernel_resources.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dad-3dheads_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_uv_texture_no_scratch_no_spills(tmp_path):
    out = subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "uv_texture.hip"), "-o", str(tmp_path / "uv_texture.o")],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert sorted(n for n in kernels if "vertex_normals_kernel" in n or "bake_kernel" in n) == sorted(kernels), list(kernels)
    assert len(kernels) == 2, list(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)  # 256-thread workgroups, at least 4 waves per SIMD


def test_uv_texture_is_built_without_contraction():
    """Bit-equality with NumPy's float64 needs every product and sum rounded on its own."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^uv_texture\.o:.*\n\t(.*)$", mk, flags=re.M)
    assert rule and "-ffp-contract=off" in rule.group(1)
