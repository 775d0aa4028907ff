"""The host index of a polygon set (pasture_amd/csrc/polygon_index.hpp) is plain C++ without HIP: the canonical edge entries, the bounding box
and the y-band directory in CSR form.  tests/cpp/test_polygon_index.cpp builds it for the sets this test writes and prints it; the program is
compiled with the address and undefined-behaviour sanitizers and run stand-alone (g++, no GPU), and what it prints is compared with the
restatement in tests/crop_ref.py: every band holds exactly the entries the restated band expression gives, sorted by polygon and then by
input order; the offsets are monotone (the program checks that itself); the refusals and their limits are honoured."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = [0, 1, 2, 7, 4096]  # 0: automatic; "more bands than edges" is added per set


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("polygon_index") / "test_polygon_index")
    # the sanitizers' runtimes are linked into the program itself: it is a stand-alone executable and needs nothing of its environment
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "pasture_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_polygon_index.cpp"),
                           "-o", exe])
    return exe


def write_set(path, polygons, with_polygons=True):
    rings = R.rings_of(polygons)
    with open(path, "w") as f:
        f.write(f"{len(rings)} {1 if with_polygons else 0}\n")
        for p, ring in rings:
            f.write(f"{p} {len(ring)}\n")
            for x, y in ring:
                f.write(f"{float(x).hex()} {float(y).hex()}\n")


def run(program, path, bands):
    r = subprocess.run([program, str(path), str(bands)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), r.stdout[-2000:] + r.stderr[-2000:]
    head, entries, lists = None, [], {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "polygons":
            head = {"polygons": int(w[1]), "entries": int(w[3]), "bands": int(w[5]), "directory": int(w[7]), "ymin": float.fromhex(w[9]), "scale": float.fromhex(w[11]),
                    "box": tuple(float.fromhex(v) for v in w[13:17])}
        elif w[0] == "entry":
            assert int(w[1]) == len(entries)
            entries.append((int(w[2]),) + tuple(float.fromhex(v) for v in w[3:7]))
        elif w[0] == "band":
            lists[int(w[1])] = [int(v) for v in w[2:]]
    return head, entries, lists


def check(program, tmp_path, polygons, bands, with_polygons=True):
    path = tmp_path / "set.txt"
    write_set(path, polygons, with_polygons)
    head, entries, lists = run(program, path, bands)
    want = R.directory(polygons if with_polygons else [[r for _, r in R.rings_of(polygons)]], bands)
    assert head["polygons"] == (len(polygons) if with_polygons else 1)
    assert head["bands"] == want["bands"] and (bands == 0 or head["bands"] == bands)
    assert head["box"] == tuple(want["box"]) and head["ymin"] == want["ymin"]
    assert head["scale"] == want["scale"] or (np.isnan(head["scale"]) and np.isnan(want["scale"]))
    # the entries: canonical, in input order, with their polygons
    assert head["entries"] == len(entries) == len(want["entries"])
    assert np.array_equal(np.array([e[1:] for e in entries]).reshape(-1, 4), want["entries"])
    assert [e[0] for e in entries] == want["polygon"].tolist()
    assert all(e[2] < e[4] for e in entries)
    # every band holds exactly the entries the restated expression gives, in input order -- which is sorted by polygon, then by input order
    got = [lists.get(b, []) for b in range(head["bands"])]
    assert got == want["lists"]
    assert head["directory"] == sum(len(v) for v in got)
    for v in got:
        keys = [(entries[e][0], e) for e in v]
        assert keys == sorted(keys)
    return head


def random_set(seed, n_polygons=5, scale=1.0, offset=(0.0, 0.0)):
    """polygons of 1 .. 3 rings of 3 .. 12 vertices; some vertices share a y (horizontal edges, entries that end on a band boundary)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_polygons):
        rings = []
        for _ in range(rng.integers(1, 4)):
            m = int(rng.integers(3, 13))
            ring = rng.random((m, 2))
            ring[:, 1] = np.round(ring[:, 1] * 16) / 16 if rng.random() < 0.5 else ring[:, 1]
            rings.append(ring * scale + np.asarray(offset))
        out.append(rings if len(rings) > 1 or rng.random() < 0.5 else rings[0])
    return out


FIXED = {
    "square": [R.rectangle(0.0, 0.0, 1.0, 1.0)],
    "closed square": [np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])],
    "hole and island": [[R.rectangle(0, 0, 9, 9), R.rectangle(2, 2, 7, 7, reverse=True), R.rectangle(4, 4, 5, 5)]],
    "bow-tie": [np.array([[0.0, 0.0], [2.0, 2.0], [2.0, 0.0], [0.0, 2.0]])],
    "all horizontal": [np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 1.0]])],
    "spike": [np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [9.0, 2.0], [4.0, 2.0], [4.0, 4.0], [0.0, 4.0]])],
    "grid": R.grid_rectangles(np.arange(5.0), np.arange(4.0)),
    "star": [R.star(64)],
    "overlap": [R.rectangle(0, 0, 4, 4), R.rectangle(2, 2, 6, 6), R.rectangle(3, -1, 5, 3)],
    "utm": [R.star(24, (5.0e5, 5.0e6), 250.0, 100.0), R.rectangle(5.0e5 - 10, 5.0e6 - 400, 5.0e5 + 10, 5.0e6 - 300)],
    "tiny extent": [np.array([[0.0, 0.0], [1.0, 5e-324], [2.0, 0.0]])],
    "huge extent": [np.array([[0.0, -1.7e308], [1.0, 1.7e308], [2.0, 0.0]])],
}


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_sets(program, tmp_path, name):
    polygons = FIXED[name]
    n_edges = sum(len(r) for _, r in R.rings_of(polygons))
    for bands in BANDS + [n_edges + 3]:
        check(program, tmp_path, polygons, bands)
    check(program, tmp_path, polygons, 7, with_polygons=False)  # polygon_of_ring NULL: one polygon made of all rings


@pytest.mark.parametrize("seed", range(6))
def test_seeded_random_sets(program, tmp_path, seed):
    polygons = random_set(seed) if seed % 2 == 0 else random_set(seed, 9, 1000.0, (5.0e5, 5.0e6))
    n_edges = sum(len(r) for _, r in R.rings_of(polygons))
    for bands in BANDS + [n_edges + 3]:
        check(program, tmp_path, polygons, bands)


def test_automatic_bands(program, tmp_path):
    """one band per eight entries, at least one"""
    assert check(program, tmp_path, FIXED["square"], 0)["bands"] == 1
    assert check(program, tmp_path, [R.star(64)], 0)["bands"] == 8
    assert check(program, tmp_path, [R.star(4096)], 0)["bands"] == 512
    assert check(program, tmp_path, FIXED["all horizontal"], 0)["entries"] == 0


def test_refusals(program):
    r = subprocess.run([program, "refusals"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refusals honoured" in r.stdout
