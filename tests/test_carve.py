"""The carver that every one-allocation call of the graph back end uses (csrc/elm_carve.hpp), on the CPU: tests/carve_check.cpp is
compiled against that header alone, with the address and undefined-behaviour sanitizers, and run as a program of its own (nothing is
loaded into this process).  On a mixed list of types and counts -- count 0 and 1, arrays of 255, 256 and 257 bytes, a uint8_t array
between two double arrays -- it checks that the size pass and the real pass give the same offsets, that every pointer is 256-byte aligned
relative to the base, that no two arrays overlap (each is written from end to end under the address sanitizer), that carved_size equals
the last offset, and that a null base yields null pointers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "elimaloc_amd", "csrc")


def test_two_passes_agree_aligned_and_disjoint(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/carve_check.cpp")
    exe = str(tmp_path / "carve_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", CSRC, os.path.join(HERE, "carve_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
