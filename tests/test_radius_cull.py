"""The cull of the fixed-radius search -- the (y, z) rows of an index's grid and the cells of a row that can hold a neighbour of a query --
is computed by pasture_amd/csrc/radius_cull.hpp, which is free of HIP: tests/cpp/test_radius_cull.cpp checks that every target the rounded
predicate accepts lies in a row and an x range the cull keeps, over random queries and grids whose edge runs from radius / 8 to 100 radius,
with dims of 1 on one, two and three axes, a query inside the grid, on a face, outside it and with its ball tangent to a cell boundary,
and on an exhaustive lattice of points one and two ulps around the sphere's knife edge and around cell boundaries; this test builds it
with the address and undefined-behaviour sanitizers and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radius_cull(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_radius_cull")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_radius_cull.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
