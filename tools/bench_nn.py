#!/usr/bin/env python3
"""Nearest neighbours between two clouds and one ICP step on synthetic points: one fresh process, warm-up, timed repetitions with device events,
medians with their spread, one JSON line.

Two pairs of clouds of the same size, each cloud in ONE columnar Position3D buffer, query and target two independent draws:
  uniform   synth_fill points in the bench's box (two seeds)
  sheet     the LiDAR-like sheet of tools/bench_clusters.py (a noisy 2-D manifold with 0.001 % far strays; two seeds)
Measured per pair: the index build (automatic cell edge); the search with max_distance = +inf (the sheet: only with --unbounded-on-sheet, its
far strays among the queries each walk thousands of rings of empty cells) and with about three mean spacings, split into
query keys + sort and search by stream events inside the call (PST_NN_TIMES=1, pst_nn_phase_times); one ICP step from the identity with the
bounded distance; with --plane also the normals set in the index (pst_nn_index_set_normals_device) and one point-to-plane step; a sweep of the cell edge around the automatic one (mean points per occupied cell aimed at 1, 2, 4, 8, 16, 32; build and unbounded
search each).  Yardsticks in the same process on the same target buffer: pst_knn_search_device with k = 3 (the nearest thing the library had:
neighbours inside ONE cloud, index rebuilt per call) and pst_calculate_bounds (one pass over the positions).

    python tools/bench_nn.py [--points 100000000] [--reps 5] [--warmup 1] [--plane] [--out profiles/nn_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_NN_TIMES"] = "1"  # read once, at the library's first search
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clusters import quartiles, sheet_cloud, timed  # noqa: E402

IDENTITY = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
SWEEP = (1, 2, 4, 8, 16, 32)


def say(text):
    print(text, file=sys.stderr, flush=True)


def measure(torch, alg, hip, query, target, n, spacing, args, unbounded=True):
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    dist = torch.empty(n, dtype=torch.float64, device="cuda")
    holder = {}

    def build(edge=0.0):
        if "index" in holder:
            holder.pop("index").destroy()
        holder["index"] = alg.NearestNeighbourIndex(target, edge)

    def search(max_distance):
        hip.nearest_neighbours_device(holder["index"]._h, query._h, None, max_distance, C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()))

    def mean_of(grid):
        return grid["n_finite"] / max(1, grid["occupied_cells"])

    out = {"mean_spacing": spacing}
    out["index_build"] = quartiles(timed(torch, build, args.warmup, args.reps)[0])
    grid = holder["index"].grid()
    out["grid"] = {"cell_edge": grid["cell_edge"], "dim": list(grid["dim"]), "n_finite": grid["n_finite"], "occupied_cells": grid["occupied_cells"],
                   "mean_points_per_occupied_cell": round(mean_of(grid), 3)}
    say(f"  index build {out['index_build']['median_ms']} ms, grid {out['grid']}")
    bounded = 3.0 * spacing
    legs = (("unbounded", float("inf")), ("bounded", bounded)) if unbounded else (("bounded", bounded),)
    if not unbounded:
        out["unbounded"] = {"skipped": "the far strays among the queries each walk thousands of rings of empty cells when nothing bounds the search (DESIGN.md 4.12); --unbounded-on-sheet runs it"}
    for name, max_distance in legs:
        t, phases = timed(torch, lambda: search(max_distance), args.warmup, args.reps, after=lambda: alg.nn_phase_times(hip))
        phases = np.median(np.asarray(phases), axis=0)
        d = dist[torch.isfinite(dist)]
        out[name] = {"max_distance": max_distance if math.isfinite(max_distance) else "inf", "call": quartiles(t),
                     "phases_ms": {"query_keys_and_sort": round(float(phases[0]), 4), "search": round(float(phases[1]), 4)},
                     "matched": int(d.numel()), "mean_distance": float(d.mean()) if d.numel() else None}
        say(f"  search {name}: {out[name]['call']['median_ms']} ms")
    sums, t12 = (C.c_double * 17)(), (C.c_double * 12)()
    t_icp = timed(torch, lambda: hip.icp_step(holder["index"]._h, query._h, IDENTITY, bounded, sums, t12), args.warmup, args.reps)[0]
    out["icp_step"] = {"max_distance": bounded, "call": quartiles(t_icp), "matched": int(sums[0]), "rms": math.sqrt(sums[16] / sums[0]) if sums[0] else None}

    if args.plane:
        # point-to-plane: the normals (0, 0, 1) for every target as an f64 [n][3] device array -- what the gather and the sums cost does not
        # depend on their values; the sheet's true normals are close to that -- set in the index, then one plane step from the identity
        normals = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        normals[:, 2] = 1.0
        t_set = timed(torch, lambda: holder["index"].set_normals(normals.data_ptr(), n), args.warmup, args.reps)[0]
        del normals
        sums35 = (C.c_double * 35)()
        t_plane = timed(torch, lambda: hip.icp_plane_step(holder["index"]._h, query._h, IDENTITY, bounded, sums35, t12), args.warmup, args.reps)[0]
        out["plane"] = {"max_distance": bounded, "set_normals": quartiles(t_set), "icp_plane_step": quartiles(t_plane), "matched": int(sums35[0]), "used": int(sums35[1]),
                        "rms": math.sqrt(sums35[32] / sums35[1]) if sums35[1] else None}
        holder["index"].set_normals(None)
        say(f"  plane: set normals {out['plane']['set_normals']['median_ms']} ms, plane step {out['plane']['icp_plane_step']['median_ms']} ms")

    # the yardsticks, on the target buffer
    d3 = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    out["knn_search_3"] = quartiles(timed(torch, lambda: hip.knn_search_device(target._h, 3, None, C.c_void_p(d3.data_ptr())), args.warmup, args.reps)[0])
    del d3
    out["calculate_bounds"] = quartiles(timed(torch, lambda: alg.calculate_bounds(target), args.warmup, args.reps)[0])
    knn = out["knn_search_3"]["median_ms"]
    say(f"  icp step {out['icp_step']['call']['median_ms']} ms, knn_search(3) {knn} ms, bounds {out['calculate_bounds']['median_ms']} ms")
    widest = "unbounded" if unbounded else "bounded"
    out["ratio_to_knn_search_3"] = {"search_bounded": round(out["bounded"]["call"]["median_ms"] / knn, 4),
                                    "build_plus_search_" + widest: round((out["index_build"]["median_ms"] + out[widest]["call"]["median_ms"]) / knn, 4),
                                    "icp_step": round(out["icp_step"]["call"]["median_ms"] / knn, 4)}
    if unbounded:
        out["ratio_to_knn_search_3"]["search_unbounded"] = round(out["unbounded"]["call"]["median_ms"] / knn, 4)
    out["ratio_to_calculate_bounds"] = {"search_" + widest: round(out[widest]["call"]["median_ms"] / out["calculate_bounds"]["median_ms"], 4)}

    # the sweep: the occupancy goes with edge^d; d from a second index at twice the automatic edge
    edge0, mean0 = grid["cell_edge"], mean_of(grid)
    build(2.0 * edge0)
    d = min(3.0, max(1.0, math.log2(max(mean_of(holder["index"].grid()), mean0 * 1.0001) / mean0)))
    sweep = []
    sweep_distance = float("inf") if unbounded else bounded
    for aim in SWEEP:
        edge = edge0 * (aim / mean0) ** (1.0 / d)
        t_build = quartiles(timed(torch, lambda: build(edge), 0, max(1, args.reps // 2))[0])
        g = holder["index"].grid()
        t, phases = timed(torch, lambda: search(sweep_distance), args.warmup, args.reps, after=lambda: alg.nn_phase_times(hip))
        sweep.append({"aimed_at": aim, "cell_edge": g["cell_edge"], "mean_points_per_occupied_cell": round(mean_of(g), 3), "index_build": t_build,
                      "search_" + widest: quartiles(t), "search_phase_ms": round(float(np.median(np.asarray(phases), axis=0)[1]), 4)})
        say(f"  sweep {aim}: mean {sweep[-1]['mean_points_per_occupied_cell']}, build {t_build['median_ms']} ms, search {sweep[-1]['search_' + widest]['median_ms']} ms")
    out["local_dimension"] = round(d, 3)
    out["edge_sweep"] = sweep
    holder.pop("index").destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--unbounded-on-sheet", action="store_true", help="also search the sheet with max_distance = +inf: its far strays walk the whole grid")
    ap.add_argument("--plane", action="store_true", help="also measure point-to-plane: normals set in the index and one plane step per cloud")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_nn.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    result = {"bench": "nn", "points": n, "seeds": [42, 43], "device": torch.cuda.get_device_name(0), "kernel_shape": alg.nn_kernel_shape(hip)}
    for name in args.clouds.split(","):
        say(name)
        if name == "uniform":
            clouds = []
            for seed in (42, 43):
                buf = pa.HashMapBuffer.new_from_layout(layout)
                buf.resize(n)
                buf.synth_fill(seed, 0)
                clouds.append(buf)
            b = alg.calculate_bounds(clouds[1])
            spacing = (float(np.prod(np.asarray(b.max()) - np.asarray(b.min()))) / n) ** (1.0 / 3.0)
            result[name] = measure(torch, alg, hip, clouds[0], clouds[1], n, spacing, args)
        elif name == "sheet":
            sheets = [sheet_cloud(torch, n, seed) for seed in (42, 43)]
            clouds = [pa.ExternalColumnsBuffer([s], layout, n) for s in sheets]
            spacing = math.sqrt(1.0e6 / n)  # the 1000 x 1000 sheet
            result[name] = measure(torch, alg, hip, clouds[0], clouds[1], n, spacing, args, unbounded=args.unbounded_on_sheet)
            del sheets
        else:
            sys.exit(f"unknown cloud {name!r}")
        del clouds
        hip.release_scratch()
        torch.cuda.empty_cache()
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
