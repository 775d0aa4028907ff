"""The ONE JSON line of bench.py on a GPU box, at a reduced size: the headline with `roofline`, `cpu_baseline` and `verified`, and the legs the
round-4 review asked to make driver-visible -- configs[2] (typed LAS-0 records -> 10 columns) and configs[4] (kNN(16) normals) with their in-run
oracle spot checks, and the north-star leg."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_carries_every_leg_and_verifies_them():
    n = 3_000_000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--points", str(n), "--steps", "4", "--warmup", "1", "--north-star-points", str(2 * n),
                        "--cpu-sample-points", str(n), "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["unit"] == "Mpoints/s" and line["dtype"] == "f64" and line["vs_baseline"] is None
    assert line["verified"] is True  # GPU AABB of the converted points == the oracle's over the same synthetic points
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and rf["algorithmic_bytes_per_point"] == 48
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0
    c2 = line["configs2_las0_to_columns"]
    assert c2["verified"] is True and c2["points"] == n and c2["algorithmic_bytes_per_point"] == 70 and 0 < c2["frac"] < 1 and c2["plan"]
    c4 = line["configs4_knn16"]
    assert c4["verified"] is True and c4["k"] == 16 and c4["ms_per_call"] > 0
    assert c4["checks"] == {"columns_equal_f64_results_narrowed": True, "neighbour_lists_checked": 48, "neighbour_lists_exact": 48}
    sc = cb["spot_checks"]
    assert sc["configs2"]["columns_compared"] == 10 and sc["configs2"]["points_compared"] == 100_000 and sc["configs4"]["fits_compared"] == 48
    ns = line["north_star_1e9"]
    assert ns["points"] == 2 * n and ns["bounds"]
    # the legs can be switched off, and the line stays whole
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--points", str(n), "--steps", "2", "--warmup", "1", "--full", "--no-extra-legs",
                        "--no-north-star", "--no-cpu-baseline"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert "configs2_las0_to_columns" not in line and "configs4_knn16" not in line and "verified" not in line and line["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_only_and_dumps_the_last_step(oracle, tmp_path):
    """Without --full the line is the headline alone; --steps is the number of timed steps.  --dump-outputs writes the last step's converted
    positions over bench.dump_sample and its AABB: equal to (p * scale) + offset of the oracle's synthetic points, and the same in a second run."""
    import numpy as np

    import bench
    from pasture_amd.buffers import HashMapBuffer
    from pasture_amd.layout import PointLayout, attributes as A
    n = 3_000_000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--points", str(n), "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "Mpoints/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
        assert line["roofline"]["frac"] > 0
        for leg in ("cpu_baseline", "verified", "configs2_las0_to_columns", "configs4_knn16", "configs4_knn16_sheet", "dropin_convert_then_bounds",
                    "chunked_rawlas_1MiB", "north_star_1e9"):
            assert leg not in line, leg
        assert sorted(os.listdir(d)) == ["Position3D.npy", "bounds.npy"]
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
        pos, box = np.load(d / "Position3D.npy"), np.load(d / "bounds.npy")
        assert pos.dtype == np.float64 and box.tolist() == [list(b) for b in line["config"]["bounds"]]
        dumps.append((pos, box))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])
    ranges = bench.dump_sample(n, 24)
    assert len(ranges) > 1 and sum(len(r) for r in ranges) == len(dumps[0][0]) < n
    src = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=oracle))
    src.resize(n)
    src.synth_fill(bench.SEED, 0)
    want = np.concatenate([src.get_attribute_range(A.POSITION_3D, r) for r in ranges]) * np.array(bench.SCALE) + np.array(bench.OFFSET)
    assert np.array_equal(dumps[0][0], want)
