"""The phase timers behind PST_<X>_TIMES=1 (pasture_amd/csrc/phase_events.hpp), switched on: the switches are read once per process, so the
calls run in a child process with all eight set -- Euclidean clusters, DBSCAN, the Poisson-disk mask, a nearest-neighbour search, height above
ground, rasterize without and with a mean (the atomic and the sorted path), the ground mask and a Morton order, each once on a small seeded
cloud with some points that are not finite.  Every *_phase_times tuple must have its documented length and hold finite, non-negative
milliseconds with a positive sum, and every result must be what the same call gives in this process with the timers off."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PST_CLUSTER_TIMES", "PST_DBSCAN_TIMES", "PST_SAMPLE_TIMES", "PST_NN_TIMES", "PST_HAG_TIMES", "PST_RASTER_TIMES", "PST_PMF_TIMES", "PST_REORDER_TIMES")
PHASES = {"clusters": 3, "dbscan": 4, "sample": 3, "nn": 2, "hag": 3, "raster": 3, "raster_mean": 3, "pmf": 3, "reorder": 3}

# run() -> {call: {"times": the call's *_phase_times right after it, "digest": sha256 over the bytes of its results}}
_SCRIPT = r"""
import hashlib, json
import numpy as np
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointLayout, attributes as A


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def cloud(hip, seed, n):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(0.0, 40.0, (n, 2)), rng.normal(0.0, 0.5, (n, 1))], axis=1)
    pts[::5, 2] += 3.0  # every fifth point stands above the rest
    pts[rng.choice(n, 3, replace=False), rng.integers(0, 3, 3)] = (np.nan, np.inf, -np.inf)
    buf = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=hip))
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    return buf, pts


def run():
    hip = pa.product_api()
    buf, pts = cloud(hip, 20240, 5000)
    other, _ = cloud(hip, 20241, 3000)
    low = (pts[:, 2] < 1.5).astype(np.uint8)  # (False for NaN)
    out = {}

    def note(name, times, *arrays):
        out[name] = {"times": list(times(hip)), "digest": digest(*arrays)}

    labels, sizes = alg.euclidean_clusters(buf, 0.9, min_size=2)
    note("clusters", alg.cluster_phase_times, labels, sizes)
    r = alg.dbscan(buf, 0.9, 4)
    note("dbscan", alg.dbscan_phase_times, r.labels, r.core, r.sizes, np.array([r.n_core, r.n_labelled]))
    mask, kept, rounds = alg.poisson_disk_mask(buf, 1.1, seed=7)  # (rounds: how many launches it took depends on the schedule, the mask does not)
    note("sample", alg.sample_phase_times, mask, np.array([kept]))
    idx, dist = alg.nearest_neighbours(other, buf, max_distance=5.0)
    note("nn", alg.nn_phase_times, idx, dist)
    hag, ground_z = alg.height_above_ground(buf, ground_mask=low, k=3, return_ground_z=True)
    note("hag", alg.hag_phase_times, hag, ground_z)
    for name, stats in (("raster", ("count", "min", "max")), ("raster_mean", ("count", "mean", "variance"))):
        ras = alg.rasterize(buf, 1.5, stats=stats)
        note(name, alg.raster_phase_times, np.array([ras.origin[0], ras.origin[1], ras.cell_size]), np.array([ras.cols, ras.rows, ras.n_members]),
             *[ras.planes[s] for s in stats])
    ground, n_ground = alg.ground_mask(buf, alg.PmfParameters(cell_size=1.0, max_window_size=9.0))
    note("pmf", alg.pmf_phase_times, ground, np.array([n_ground]))
    order, keys = alg.morton_order(buf, return_keys=True)
    note("reorder", alg.reorder_phase_times, order, keys)
    return out
"""


@pytest.mark.gpu
def test_phase_timers_switched_on(hip):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **{name: "1" for name in SWITCHES})
    child = subprocess.run([sys.executable, "-c", _SCRIPT + "\nprint('RESULT ' + json.dumps(run()))\n"], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout + child.stderr
    timed = json.loads([line for line in child.stdout.splitlines() if line.startswith("RESULT ")][-1][len("RESULT "):])
    scope = {}
    exec(_SCRIPT, scope)
    plain = scope["run"]()  # the same calls in this process
    assert set(timed) == set(plain) == set(PHASES)
    for name, phases in PHASES.items():
        times = timed[name]["times"]
        print(name, times)
        assert len(times) == phases, (name, times)
        assert all(np.isfinite(t) and t >= 0.0 for t in times), (name, times)
        assert sum(times) > 0.0, (name, times)
        assert timed[name]["digest"] == plain[name]["digest"], f"{name}: the result with the timers on differs from the result with them off"
        if not any(os.environ.get(s, "")[:1] not in ("", "0") for s in SWITCHES):
            assert plain[name]["times"] == [0.0] * phases, (name, plain[name]["times"])
