"""The XY grid of pst_height_above_ground_device is sized on the host by pasture_amd/csrc/hag_grid.hpp, which is free of HIP:
tests/cpp/test_hag_grid.cpp checks dims and bits for zero-extent axes and a single point, extents that force the doubling on either limit, the
largest coordinate landing in cell dim - 1 and a given edge kept as given; this test builds it with the address and undefined-behaviour sanitizers
and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hag_grid(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_hag_grid")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_hag_grid.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
