"""The scratch carver of the RANSAC, outlier and cluster entry points (pasture_amd/csrc/scratch_layout.hpp) is host-only and free of HIP: every
region starts on a 256-byte boundary, regions never overlap, an empty region takes no room.  tests/cpp/test_scratch_layout.cpp asserts that, and
the fact the cluster call's 4-byte halves rely on; this test builds it with the address and undefined-behaviour sanitizers and runs it (g++, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_layout(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_scratch_layout")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_scratch_layout.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
