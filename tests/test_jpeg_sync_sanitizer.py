"""CPU: the host half of the piece-wise JPEG entropy stage under AddressSanitizer and UndefinedBehaviorSanitizer. The stand-alone
program tests/jpeg_sync_sanitize_main.cpp (its own `main`, plain C++ over csrc/jpeg_sync.hpp and csrc/jpeg_entropy.hpp, nothing
preloaded, no GPU) runs every truncation and every single-bit flip of four small files through the routines the kernels run, each
file in a heap block of exactly its size, and must end clean and in agreement with the serial walk."""
import os
import shutil
import subprocess

import pytest

from jpeg_cases import jpeg, picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILER = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
STATIC = ["-static-libasan", "-static-libubsan"] if COMPILER.endswith("g++") and "clang" not in COMPILER else []  # clang links them statically


@pytest.mark.skipif(not os.path.exists(COMPILER), reason="no host C++ compiler")
def test_truncations_and_bit_flips_end_clean_under_the_sanitizers(tmp_path):
    program = str(tmp_path / "jpeg_sync_sanitize")
    built = subprocess.run([COMPILER, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            *STATIC, os.path.join(ROOT, "tests", "jpeg_sync_sanitize_main.cpp"), "-o", program], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    files = [jpeg(picture((8, 8, 3), 4), quality=90), jpeg(picture((17, 9, 3), 2), quality=75, subsampling=2, restart_marker_blocks=1),
             jpeg(picture((12, 20), 3), quality=50), jpeg(picture((16, 16, 3), 6), quality=100, subsampling=0)]  # the last: several pieces of 16 bytes
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / f"{k}.jpg"))
        with open(paths[-1], "wb") as out:
            out.write(f)
    ran = subprocess.run([program, *paths], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout[-1000:], ran.stderr[-3000:])
    counts = [int(w) for w in ran.stdout.split() if w.isdigit()]
    assert counts[0] == sum(1 + 9 * len(f) for f in files) and 0 < counts[1] < counts[0] and counts[2] > 1000, ran.stdout
