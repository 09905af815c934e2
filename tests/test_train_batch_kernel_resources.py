"""CPU: the training-batch keypoint kernel (csrc/train_batch.hip) has no scratch and no spills, and its unit is built with
-ffp-contract=off. Compiled for gfx950 with `-Rpass-analysis=kernel-resource-usage`, as in
tests/test_train_objective_kernel_resources.py."""
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
def test_train_batch_no_scratch_no_spills(tmp_path):
    out = subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "train_batch.hip"), "-o", str(tmp_path / "tb.o")],
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
    assert len(kernels) == 1 and "gt_keypoints_kernel" in next(iter(kernels)), list(kernels)
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) == 0, (name, k)
        assert int(k["VGPRs"]) <= 64, (name, k)


def test_train_batch_is_built_without_contraction():
    """The barycentric products, the float64 scale-and-pad and the projection sums stay unfused."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^train_batch\.o:.*\n\t(.*)$", mk, flags=re.M)
    assert rule and "-ffp-contract=off" in rule.group(1)
    assert re.search(r"^OBJS\s*:=.*\btrain_batch\.o\b", mk, flags=re.M)


def test_projection_arithmetic_has_one_copy():
    """project_vertices_kernel and the training-batch kernel share projection_math.hpp; neither restates the sums."""
    for fn in ("projection.hip", "train_batch.hip"):
        src = open(os.path.join(CSRC, fn)).read()
        assert '#include "projection_math.hpp"' in src, fn
        assert "mv[4 * i]" not in src and "pm[4 * i]" not in src, fn
