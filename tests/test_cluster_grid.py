"""The 3-D grid of the cluster index (Euclidean clusters, DBSCAN, Poisson-disk subsampling, the nearest-neighbour index) is sized on the host by
pasture_amd/csrc/cluster_grid.hpp, which is free of HIP: tests/cpp/test_cluster_grid.cpp checks dims and bits for a single point and zero-extent
axes, the edge of exactly tolerance * (1 + 2^-20), quotients just below and at 2^21 - 1 (no doubling, one doubling), the largest coordinate
landing in cell dim - 1, the bits (dim <= 2^bits < 2 dim, 63 in all at the most), an extent that overflows f64 and a given edge kept as given;
this test builds it with the address and undefined-behaviour sanitizers and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_grid(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_cluster_grid")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_cluster_grid.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
