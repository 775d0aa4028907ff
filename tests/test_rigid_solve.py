"""The rigid solve of the ICP step (pasture_amd/csrc/rigid_solve.hpp) is host-only and free of HIP: Horn's unit quaternion from a cyclic Jacobi
eigen-solver, which can only return proper rotations.  tests/cpp/test_rigid_solve.cpp checks it on known rotations, on reflected, rank-1 and
rank-0 inputs and on random ones; this test builds it with the address and undefined-behaviour sanitizers and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rigid_solve(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_rigid_solve")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_rigid_solve.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
