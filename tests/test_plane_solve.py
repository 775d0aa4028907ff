"""The solve of the point-to-plane ICP step (pasture_amd/csrc/plane_solve.hpp) is host-only and free of HIP: the minimum-norm solution of the
6 x 6 normal equations through the cyclic Jacobi eigen-solver it shares with rigid_solve.hpp, and Rodrigues' formula.
tests/cpp/test_plane_solve.cpp checks it on known motions, on rank-deficient, zero and non-finite systems, the Jacobi solver on random symmetric
matrices and the rotation over the whole range of angles; this test builds it with the address and undefined-behaviour sanitizers and runs it
(g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_solve(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_plane_solve")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_plane_solve.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
