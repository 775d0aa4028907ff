#!/usr/bin/env python3
"""Fixed-radius neighbour search on synthetic clouds: every leg in a fresh child process under its own time limit, warm-up, timed
repetitions with device events, medians with their spread, one JSON line.

Legs (each cloud in ONE columnar Position3D buffer, searched against an index over itself):
  uniform, sheet   `--points` points drawn uniformly in a cube whose mean spacing is 1 / the LiDAR-like sheet of tools/bench_clusters.py, the
                   radius at about 8 neighbours: the index build, the count call alone, the full search with and without distances, the four
                   phases (PST_RADIUS_TIMES=1, pst_radius_phase_times), entries per second, the share of entries in lists above the LDS cap
  dense            `--dense-points` uniform points at about 64 neighbours (below the 2^32 - 16 entries of one call)
  edge_sweep       `--sweep-points` uniform points at about 8 neighbours, the index's cell edge from radius / 4 to 4 radius
Yardsticks in the same process on the same buffers: pst_knn_search_device at k = 8 (it writes the same number of entries),
pst_radius_outlier_mask, the count phase of pst_dbscan at min_points = 16 (PST_DBSCAN_TIMES=1), pst_calculate_bounds.

    python tools/bench_radius.py [--points 100000000] [--dense-points 20000000] [--sweep-points 20000000] [--reps 3] [--warmup 1]
                                 [--legs uniform,sheet,dense,edge_sweep] [--limit 900] [--out profiles/radius_1e8.json]
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

EDGE_FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)


def say(text):
    print(text, file=sys.stderr, flush=True)


def make_cloud(torch, kind, n):
    """(points tensor, radius of a ball that holds about `aim` points with aim = 1)"""
    from bench_clusters import sheet_cloud
    if kind == "sheet":
        return sheet_cloud(torch, n, 42), lambda aim: math.sqrt(aim * 1.0e6 / (math.pi * n))
    g = torch.Generator(device="cuda")
    g.manual_seed(42)
    side = n ** (1.0 / 3.0)
    return torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g) * side, lambda aim: (aim * 3.0 / (4.0 * math.pi)) ** (1.0 / 3.0)


def child(args):
    """One leg; prints its JSON object on the last line of stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_radius.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A
    from bench_clusters import quartiles, timed

    hip = pa.product_api()
    leg = args.child
    kind = "sheet" if leg == "sheet" else "uniform"
    n = {"dense": args.dense_points, "edge_sweep": args.sweep_points}.get(leg, args.points)
    aim = 64.0 if leg == "dense" else 8.0
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    cloud, radius_for = make_cloud(torch, kind, n)
    radius = radius_for(aim)
    buf = pa.ExternalColumnsBuffer([cloud], layout, n)
    out = {"points": n, "radius": radius, "neighbours_aimed_at": aim}
    cap = pa.radius_kernel_shape()["sort_cap"]
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    total = C.c_uint64()

    def measure(index, with_yardsticks):
        row = {}
        g = index.grid()
        row["grid"] = {"cell_edge": g["cell_edge"], "dim": list(g["dim"]), "mean_points_per_occupied_cell": round(g["n_finite"] / max(1, g["occupied_cells"]), 3)}

        def count():
            hip.radius_neighbour_counts_device(index._h, buf._h, None, radius, C.c_void_p(counts.data_ptr()), C.byref(total))

        t, phases = timed(torch, count, args.warmup, args.reps, after=lambda: alg.radius_phase_times(hip))
        row["count_call"] = quartiles(t)
        p = np.median(np.asarray(phases), axis=0)
        row["count_call_phases_ms"] = {"query_keys_and_sort": round(float(p[0]), 4), "count_and_scan": round(float(p[1]), 4)}
        entries = total.value
        row["entries"] = entries
        row["neighbours_per_query"] = round(entries / n, 3)
        if entries >= 0xFFFFFFF0:
            row["search"] = "not measured: more than 2^32 - 17 entries"
            return row
        indices = torch.empty(entries, dtype=torch.int32, device="cuda")
        for name, with_distances in (("search_with_distances", True), ("search_without_distances", False)):
            distances = torch.empty(entries, dtype=torch.float64, device="cuda") if with_distances else None

            def search():
                hip.radius_search_device(index._h, buf._h, None, radius, C.c_void_p(offsets.data_ptr()), C.c_void_p(indices.data_ptr()),
                                         C.c_void_p(distances.data_ptr()) if with_distances else None, entries, C.byref(total))

            t, phases = timed(torch, search, args.warmup, args.reps, after=lambda: alg.radius_phase_times(hip))
            p = np.median(np.asarray(phases), axis=0)
            q = quartiles(t)
            row[name] = {"call": q, "entries_per_second": round(entries / (q["median_ms"] * 1e-3)),
                         "phases_ms": dict(zip(("query_keys_and_sort", "count_and_scan", "fill", "order"), (round(float(v), 4) for v in p)))}
            say(f"    {name}: {q}")
            del distances
        lengths = offsets[1:] - offsets[:-1]
        row["share_of_entries_in_lists_above_the_cap"] = round(float(lengths[lengths > cap].sum()) / max(1, entries), 6)
        row["longest_list"] = int(lengths.max())
        del indices
        if with_yardsticks:
            knn = torch.empty((n, 8), dtype=torch.int32, device="cuda")
            dist = torch.empty((n, 8), dtype=torch.float64, device="cuda")
            y = {"knn_search_k8": quartiles(timed(torch, lambda: hip.knn_search_device(buf._h, 8, C.c_void_p(knn.data_ptr()), C.c_void_p(dist.data_ptr())), args.warmup, args.reps)[0])}
            del knn, dist
            mask = torch.empty(n, dtype=torch.uint8, device="cuda")
            kept = C.c_uint64()
            y["radius_outlier_mask"] = quartiles(timed(torch, lambda: hip.radius_outlier_mask(buf._h, radius, 8, C.c_void_p(mask.data_ptr()), 0, C.byref(kept)), args.warmup, args.reps)[0])
            labels = torch.empty(n, dtype=torch.int32, device="cuda")
            c3 = (C.c_uint64 * 3)()
            t, phases = timed(torch, lambda: hip.dbscan(buf._h, radius, 16, C.c_void_p(labels.data_ptr()), C.c_void_p(mask.data_ptr()), 0, None, 0, c3), args.warmup, args.reps,
                              after=lambda: alg.dbscan_phase_times(hip))
            y["dbscan_min_points_16"] = {"call": quartiles(t), "count_phase_ms": round(float(np.median(np.asarray(phases), axis=0)[1]), 4)}
            y["calculate_bounds"] = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
            row["yardsticks"] = y
            cm = row["count_call"]["median_ms"]
            row["ratios"] = {"count_call_to_dbscan_count_phase": round(cm / max(y["dbscan_min_points_16"]["count_phase_ms"], 1e-9), 3),
                             "count_call_to_radius_outlier_mask": round(cm / y["radius_outlier_mask"]["median_ms"], 3),
                             "search_with_distances_to_knn_search_k8": round(row["search_with_distances"]["call"]["median_ms"] / y["knn_search_k8"]["median_ms"], 3),
                             "count_call_to_calculate_bounds": round(cm / y["calculate_bounds"]["median_ms"], 3)}
        return row

    if leg == "edge_sweep":
        out["sweep"] = []
        for f in EDGE_FACTORS:
            index = alg.NearestNeighbourIndex(buf, f * radius)
            row = {"cell_edge_in_radii": f, **measure(index, False)}
            index.destroy()
            out["sweep"].append(row)
            say(f"  cell edge {f} radius: count {row['count_call']}")
    else:
        holder = {}

        def build():
            if "index" in holder:
                holder.pop("index").destroy()
            holder["index"] = alg.NearestNeighbourIndex(buf)

        out["index_build"] = quartiles(timed(torch, build, 0, max(1, args.reps // 2))[0])
        out.update(measure(holder["index"], True))
        holder["index"].destroy()
    del cloud
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--dense-points", type=int, default=20_000_000)
    ap.add_argument("--sweep-points", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="uniform,sheet,dense,edge_sweep")
    ap.add_argument("--limit", type=int, default=900, help="seconds one child process may take; after a child that fails or runs out of time no other is started")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    result = {"bench": "radius_search", "seed": 42}
    base = [sys.executable, os.path.abspath(__file__), "--points", str(args.points), "--dense-points", str(args.dense_points), "--sweep-points", str(args.sweep_points),
            "--reps", str(args.reps), "--warmup", str(args.warmup)]
    ok = True
    for name in args.legs.split(","):
        if not ok:
            result[name] = {"skipped": "an earlier leg failed or ran out of time"}
            continue
        say(name)
        try:
            r = subprocess.run(base + ["--child", name], env=dict(os.environ, PST_RADIUS_TIMES="1", PST_DBSCAN_TIMES="1"), stdout=subprocess.PIPE, text=True, timeout=args.limit)
            ok = r.returncode == 0
            result[name] = json.loads(r.stdout.strip().splitlines()[-1]) if ok else {"failed": r.returncode}
        except subprocess.TimeoutExpired:
            ok = False
            result[name] = {"failed": f"no result within {args.limit} s"}
    if ok:
        try:
            import pasture_amd as pa
            result["kernel_shape"] = pa.radius_kernel_shape()
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
