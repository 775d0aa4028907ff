#!/usr/bin/env python3
"""M3C2 change detection on synthetic clouds: per cloud kind one fresh child process under its own time limit, warm-up, timed repetitions with
device events, medians with their spread, one JSON line.

Two pairs of clouds of `--points` points each, each cloud in ONE columnar Position3D buffer, the second an independent draw displaced by 0.3
mean spacings along z:
  uniform   points drawn uniformly in a cube whose mean spacing is 1
  sheet     the LiDAR-like sheet of tools/bench_clusters.py (a noisy 2-D manifold with 0.001 % far strays)
Core points: the first cloud thinned by subsample_min_distance to about `--cores` points.  Measured per pair: the two index builds; then, for
R at about 2, 4 and 8 mean spacings with L = 10 R and for vertical (0, 0, 1) and diagonal (1, 1, 1) normals handed over as d_normals, the call,
its three phases (PST_M3C2_TIMES=1, pst_m3c2_phase_times) and -- in one more, untimed call of a second child started with PST_M3C2_WORK=1 --
the three work counters (rows searched, candidates tested, members); once per pair the nearest-normal mode (normals (0, 0, 1) set in the
reference index) at the smallest R.  Yardsticks in the same process on the same buffers: pst_nearest_neighbours_device of the core points in
the reference index, pst_radius_outlier_mask of the first cloud at each R (one repetition: it is the slowest line), pst_calculate_bounds.

    python tools/bench_m3c2.py [--points 100000000] [--cores 10000000] [--reps 3] [--warmup 1] [--limit 900] [--out profiles/m3c2_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SPACINGS = (2.0, 4.0, 8.0)
NORMALS = {"vertical": (0.0, 0.0, 1.0), "diagonal": (1.0, 1.0, 1.0)}


def say(text):
    print(text, file=sys.stderr, flush=True)


def make_pair(torch, pa, kind, n, layout):
    """(first, second, mean spacing, local dimension, what keeps the tensors alive)"""
    from bench_clusters import sheet_cloud
    if kind == "uniform":
        side = n ** (1.0 / 3.0)
        clouds = []
        for seed in (42, 43):
            g = torch.Generator(device="cuda")
            g.manual_seed(seed)
            clouds.append(torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g) * side)
        spacing, dimension = 1.0, 3
    elif kind == "sheet":
        clouds = [sheet_cloud(torch, n, seed) for seed in (42, 43)]
        spacing, dimension = math.sqrt(1.0e6 / n), 2
    else:
        sys.exit(f"unknown cloud {kind!r}")
    clouds[1][:, 2] += 0.3 * spacing
    return [pa.ExternalColumnsBuffer([c], layout, n) for c in clouds], spacing, dimension, clouds


def child(args):
    """One pair of clouds; prints its JSON object on the last line of stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_m3c2.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A
    from bench_clusters import quartiles, timed

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    (first, second), spacing, dimension, keep = make_pair(torch, pa, args.child, n, layout)
    counting = bool(os.environ.get("PST_M3C2_WORK"))
    out = {"mean_spacing": spacing}
    thin = 0.75 * spacing * (n / args.cores) ** (1.0 / dimension)
    core, _ = alg.subsample_min_distance(first, thin, seed=1, out_buffer_type=pa.HashMapBuffer)
    m = core.len()
    out["core_points"] = {"count": m, "min_distance": thin}
    say(f"  {m} core points")
    holder = {}

    def build(which, buf):
        if which in holder:
            holder.pop(which).destroy()
        holder[which] = alg.NearestNeighbourIndex(buf)

    reps = 0 if counting else args.reps
    if not counting:
        out["index_build"] = {w: quartiles(timed(torch, lambda w=w, b=b: build(w, b), 0, max(1, reps // 2))[0]) for w, b in (("reference", first), ("compared", second))}
    else:
        build("reference", first)
        build("compared", second)
    ref, cmp = holder["reference"], holder["compared"]
    g = ref.grid()
    out["reference_grid"] = {"cell_edge": g["cell_edge"], "dim": list(g["dim"]), "mean_points_per_occupied_cell": round(g["n_finite"] / max(1, g["occupied_cells"]), 3)}
    dist = torch.empty(m, dtype=torch.float64, device="cuda")
    sig = torch.empty(m, dtype=torch.uint8, device="cuda")
    counts = torch.empty((m, 2), dtype=torch.int32, device="cuda")
    normals = torch.empty((m, 3), dtype=torch.float64, device="cuda")
    nsig = C.c_uint64()

    def call(radius, normals_ptr):
        hip.m3c2_device(ref._h, cmp._h, core._h, C.c_void_p(normals_ptr or None), radius, 10.0 * radius, 4, 0.0, 0, C.c_void_p(dist.data_ptr()), None,
                        C.c_void_p(sig.data_ptr()), C.c_void_p(counts.data_ptr()), None, None, C.byref(nsig))

    def leg(radius, normals_ptr):
        if counting:
            call(radius, normals_ptr)
            w = alg.m3c2_work(hip)
            return {"work": w, "candidates_per_member": round(w["candidates"] / max(1, w["members"]), 3), "members_per_core_point_and_cloud": round(w["members"] / (2.0 * m), 2)}
        t, phases = timed(torch, lambda: call(radius, normals_ptr), args.warmup, reps, after=lambda: alg.m3c2_phase_times(hip))
        p = np.median(np.asarray(phases), axis=0)
        c = counts.cpu().numpy().view(np.uint32)
        return {"call": quartiles(t), "phases_ms": {"normal_lookup": round(float(p[0]), 4), "core_keys_and_sort": round(float(p[1]), 4), "cylinder_pass": round(float(p[2]), 4)},
                "significant": nsig.value, "measured": int(((c[:, 0] >= 4) & (c[:, 1] >= 4)).sum()), "median_distance": float(torch.nanmedian(dist))}

    out["sweep"] = []
    for k in SPACINGS:
        radius = k * spacing
        for name, direction in NORMALS.items():
            normals[:] = torch.tensor(direction, dtype=torch.float64, device="cuda")
            row = {"radius_in_spacings": k, "radius": radius, "max_depth": 10.0 * radius, "normals": name}
            row.update(leg(radius, normals.data_ptr()))
            out["sweep"].append(row)
            say(f"  R = {k} spacings, {name}: {row.get('call', row.get('work'))}")
    # the nearest-normal mode: (0, 0, 1) for every reference point, set in the index
    up = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    up[:, 2] = 1.0
    ref.set_normals(up.data_ptr(), n)
    del up
    out["nearest_normal_mode"] = {"radius_in_spacings": SPACINGS[0], **leg(SPACINGS[0] * spacing, 0)}
    if not counting:
        # the yardsticks
        t_nn = quartiles(timed(torch, lambda: hip.nearest_neighbours_device(ref._h, core._h, None, float("inf"), None, C.c_void_p(dist.data_ptr())), args.warmup, reps)[0])
        out["nearest_neighbours_of_the_core_points"] = t_nn
        mask = torch.empty(n, dtype=torch.uint8, device="cuda")
        kept = C.c_uint64()
        out["radius_outlier_mask_of_the_first_cloud"] = {}
        for k in SPACINGS:
            t = timed(torch, lambda: hip.radius_outlier_mask(first._h, k * spacing, 8, C.c_void_p(mask.data_ptr()), 0, C.byref(kept)), 0, 1)[0]
            out["radius_outlier_mask_of_the_first_cloud"][f"{k}_spacings"] = quartiles(t)
            say(f"  radius outlier mask at {k} spacings: {t[0]:.1f} ms")
        out["calculate_bounds_of_the_first_cloud"] = quartiles(timed(torch, lambda: alg.calculate_bounds(first), args.warmup, reps)[0])
        for row in out["sweep"]:
            row["ratio_to_nearest_neighbours"] = round(row["call"]["median_ms"] / t_nn["median_ms"], 3)
    for index in holder.values():
        index.destroy()
    del keep
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--cores", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--limit", type=int, default=900, help="seconds one child process may take; after a child that fails or runs out of time no other is started")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    result = {"bench": "m3c2", "points": args.points, "cores_aimed_at": args.cores, "seeds": [42, 43], "spacings": list(SPACINGS)}
    base = [sys.executable, os.path.abspath(__file__), "--points", str(args.points), "--cores", str(args.cores), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    ok = True
    for name in args.clouds.split(","):
        result[name] = {}
        for part, extra in (("timed", {"PST_M3C2_TIMES": "1"}), ("work", {"PST_M3C2_WORK": "1"})):
            if not ok:
                result[name][part] = {"skipped": "an earlier step failed or ran out of time"}
                continue
            say(f"{name} ({part})")
            try:
                r = subprocess.run(base + ["--child", name], env=dict(os.environ, **extra), stdout=subprocess.PIPE, text=True, timeout=args.limit)
                ok = r.returncode == 0
                result[name][part] = json.loads(r.stdout.strip().splitlines()[-1]) if ok else {"failed": r.returncode}
            except subprocess.TimeoutExpired:
                ok = False
                result[name][part] = {"failed": f"no result within {args.limit} s"}
    if ok:
        try:
            import pasture_amd as pa
            result["kernel_shape"] = pa.m3c2_kernel_shape()
        except Exception:  # (the parent never touches the GPU; the shape is a host call)
            pass
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
