"""The block layout both cell grids share (csrc/elm_grid_layout.hpp) against a naive reference, on the CPU: tests/grid_layout_check.cpp is
compiled against that header alone, with the address and undefined-behaviour sanitizers, and run as a program of its own (nothing is
loaded into this process).  It compares start[], the blocks and the slot-to-point table with a stable sort of (entry, input index) for
entries of 0, 1, 3, 4, 5 and 9 points, all points in one entry, no points at all, the last entry occupied and entry numbers in
descending input order, and checks the padding (block 0, every unused slot), the four trailing entries and that every point appears
exactly once."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "elimaloc_amd", "csrc")


def test_layout_equals_the_stable_sort(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/grid_layout_check.cpp")
    exe = str(tmp_path / "grid_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", CSRC, os.path.join(HERE, "grid_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout
