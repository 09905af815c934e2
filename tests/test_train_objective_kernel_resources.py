"""CPU: the training-objective kernels (csrc/train_objective.hip) stay free of scratch and spills, within 64 KB of LDS, and the
unit is built with -ffp-contract=off. Compiled for gfx950 with `-Rpass-analysis=kernel-resource-usage`, as in
tests/test_uv_texture_kernel_resources.py."""
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
KERNELS = ("heatmap_encode_kernel", "iou_terms_kernel", "iou_finish_kernel", "iou_grad_kernel", "visibility_loss_kernel",
           "keypoint_err_kernel", "keypoint_finish_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_train_objective_no_scratch_no_spills(tmp_path):
    out = subprocess.run([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "train_objective.hip"), "-o", str(tmp_path / "to.o")],
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
    assert all(any(k in n for k in KERNELS) for n in kernels), list(kernels)
    assert all(any(k in n for n in kernels) for k in KERNELS), list(kernels)
    assert len(kernels) == 2 + 8 + 1 + 4 + 1 + 2 + 1, list(kernels)  # template instances
    for name, k in kernels.items():
        assert int(k["ScratchSize"]) == 0, (name, k)
        assert int(k["VGPRs Spill"]) == 0 and int(k["SGPRs Spill"]) == 0, (name, k)
        assert int(k["LDS Size"]) <= 64 * 1024, (name, k)
        assert int(k["VGPRs"]) <= 128, (name, k)


def test_train_objective_is_built_without_contraction():
    """The reference's fp32 arithmetic has no FMAs (the floor-divide rule and the fp32 products of the landmark loss)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^train_objective\.o:.*\n\t(.*)$", mk, flags=re.M)
    assert rule and "-ffp-contract=off" in rule.group(1)
    assert re.search(r"^OBJS\s*:=.*\btrain_objective\.o\b", mk, flags=re.M)
