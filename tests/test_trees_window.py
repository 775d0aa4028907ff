"""The window of the local-maximum filter (pst_tree_tops_device) -- its radius from a height and the cells of the candidate grid it can
touch -- is computed by pasture_amd/csrc/trees_window.hpp, which is free of HIP: tests/cpp/test_trees_window.cpp checks the radii at the
clamps, with b < 0 and with an infinite r_max, the cell ranges at the grid's first and last cell and at dims of 1, and on an exhaustive
lattice of points one and two ulps around the knife edge that the range covers the cell of every point the rounded predicate accepts; this
test builds it with the address and undefined-behaviour sanitizers and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trees_window(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_trees_window")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_trees_window.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
