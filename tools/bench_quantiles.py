#!/usr/bin/env python3
"""Quantiles per cell and per segment: per leg one fresh child process under its own time limit (two, in fact: the second with
PST_QUANTILES_GENERAL=1, every group on the general two-sort path), warm-up, timed repetitions with device events, medians with their
spread, one JSON line.

The legs, on ONE columnar Position3D buffer each (z uniform in [0, 30): the heights):
  cells_random    `--points` points uniform over a square with 10 points per 1 m cell, as drawn
  cells_scanline  the same points in row-major cell order
  trees           `--points` points, 10^5 segments (70 % of the points labelled), as drawn
  regions         `--points` points, 2 * 10^6 segments of about 40 (80 % labelled)
  one_group       `--points` / 10 points, every one in segment 0
Measured per leg: the call with probs = (0.5, 0.95) and one threshold (2 m), the call with 19 probabilities, the four phases of the first
(PST_QUANTILES_TIMES=1, pst_quantiles_phase_times).  Yardsticks in the same process on the same buffer, all of them calls the library had
before: pst_rasterize with all five statistics (cell legs) or pst_segment_statistics with all eight (segment legs), and pst_calculate_bounds.

    python tools/bench_quantiles.py [--points 100000000] [--reps 3] [--warmup 1] [--limit 600] [--out profiles/quantiles_1e8.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LEGS = ("cells_random", "cells_scanline", "trees", "regions", "one_group")
REQUESTS = {"p50_p95_cover": ((0.5, 0.95), (2.0,)), "nineteen": (tuple(round(0.05 * k, 2) for k in range(1, 20)), ())}
PHASES = ("keys_sort_directory", "gather", "counts_and_small_groups", "large_groups")


def say(text):
    print(text, file=sys.stderr, flush=True)


def child(args):
    """One leg; prints its JSON object on the last line of stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_quantiles.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A
    from bench_clusters import quartiles, timed

    hip = pa.product_api()
    leg, general = args.child, bool(os.environ.get("PST_QUANTILES_GENERAL"))
    n = args.points // 10 if leg == "one_group" else args.points
    g = torch.Generator(device="cuda")
    g.manual_seed(42)
    cells = leg.startswith("cells")
    side = max(1.0, float(int((n / 10.0) ** 0.5)))
    cloud = torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g) * torch.tensor([side, side, 30.0], device="cuda", dtype=torch.float64)
    if leg == "cells_scanline":
        cloud = cloud[torch.argsort(cloud[:, 1].floor() * side + cloud[:, 0].floor(), stable=True)].contiguous()
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    buf = pa.ExternalColumnsBuffer([cloud], layout, n)
    members = C.c_uint64()
    if cells:
        dim = (int(side), int(side))
        G = dim[0] * dim[1]
        c_origin, c_dim = (C.c_double * 2)(0.0, 0.0), (C.c_uint32 * 2)(*dim)
    else:
        S, labelled = {"trees": (100_000, 0.7), "regions": (2_000_000, 0.8), "one_group": (1, 1.0)}[leg]
        labels = torch.randint(0, S, (n,), device="cuda", generator=g)
        labels[torch.rand(n, device="cuda", generator=g) >= labelled] = -1
        lab32 = labels.to(torch.int32)  # (-1 becomes 0xFFFFFFFF: the u32 bit pattern in an int32 tensor)
        G = S
        del labels
    planes = torch.empty((20, G), dtype=torch.float64, device="cuda")

    def quantiles(probs, thr):
        p, t = (C.c_double * max(1, len(probs)))(*probs), (C.c_double * max(1, len(thr)))(*thr)
        if cells:
            hip.rasterize_quantiles(buf._h, None, None, 1.0, c_origin, c_dim, p, len(probs), 0, t, len(thr), C.c_void_p(planes.data_ptr()), 0, None, None, C.byref(members))
        else:
            hip.segment_quantiles(buf._h, C.c_void_p(lab32.data_ptr()), G, None, None, p, len(probs), 0, t, len(thr), C.c_void_p(planes.data_ptr()), 0, C.byref(members))

    row = {"points": n, "groups": G, "general_path_forced": general}
    quantiles(*REQUESTS["p50_p95_cover"])  # (untimed: the library must see the cloud torch made before anything is measured on it)
    row["members"] = members.value
    row["largest_group"] = int(planes[0].max().item())
    for name, (probs, thr) in REQUESTS.items():
        times, phases = timed(torch, lambda: quantiles(probs, thr), args.warmup, args.reps, after=lambda: alg.quantiles_phase_times(hip))
        row[name] = quartiles(times)
        if name == "p50_p95_cover":
            row["phases_ms"] = dict(zip(PHASES, (round(float(v), 4) for v in np.median(np.asarray(phases), axis=0))))
    if not general:  # the yardsticks: calls the library had before, on the same buffer
        if cells:
            raster = torch.empty((5, dim[1], dim[0]), dtype=torch.float64, device="cuda")
            table = lambda: alg.rasterize(buf, 1.0, ("count", "min", "max", "mean", "variance"), origin=(0.0, 0.0), dim=dim, device_out_ptr=raster.data_ptr())
            what = "rasterize_all_five"
        else:
            bits = alg.segment_stats_bits(alg.SEGMENT_STATS)
            stats = torch.empty((alg.segment_planes(bits), G), dtype=torch.float64, device="cuda")
            table = lambda: hip.segment_statistics(buf._h, C.c_void_p(lab32.data_ptr()), G, None, None, bits, C.c_void_p(stats.data_ptr()), None, 0, C.byref(members))
            what = "segment_statistics_all"
        row["yardsticks"] = {what: quartiles(timed(torch, table, args.warmup, args.reps)[0]),
                             "calculate_bounds": quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])}
    say(f"  {leg}{' (general path forced)' if general else ''}: {row}")
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--limit", type=int, default=600, help="seconds one child process may take; after a child that fails or runs out of time no other is started")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    result = {"bench": "quantiles", "points": args.points, "seed": 42}
    base = [sys.executable, os.path.abspath(__file__), "--points", str(args.points), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    ok = True
    for leg in args.legs.split(","):
        result[leg] = {}
        for key, switch in (("library", {}), ("general_path_forced", {"PST_QUANTILES_GENERAL": "1"})):
            if not ok:
                result[leg][key] = {"skipped": "an earlier leg failed or ran out of time"}
                continue
            say(f"{leg} {key}")
            try:
                r = subprocess.run(base + ["--child", leg], env=dict(os.environ, PST_QUANTILES_TIMES="1", **switch), stdout=subprocess.PIPE, text=True, timeout=args.limit)
                ok = r.returncode == 0
                result[leg][key] = json.loads(r.stdout.strip().splitlines()[-1]) if ok else {"failed": r.returncode}
            except subprocess.TimeoutExpired:
                ok = False
                result[leg][key] = {"failed": f"no result within {args.limit} s"}
        lib, gen = result[leg]["library"], result[leg]["general_path_forced"]
        if "p50_p95_cover" in lib and "p50_p95_cover" in gen:
            ratios = {"general_to_library": round(gen["p50_p95_cover"]["median_ms"] / lib["p50_p95_cover"]["median_ms"], 3),
                      "nineteen_to_p50_p95_cover": round(lib["nineteen"]["median_ms"] / lib["p50_p95_cover"]["median_ms"], 3)}
            for name, t in lib["yardsticks"].items():
                ratios["library_to_" + name] = round(lib["p50_p95_cover"]["median_ms"] / t["median_ms"], 3)
            result[leg]["ratios"] = ratios
    try:
        import pasture_amd as pa
        result["kernel_shape"] = pa.quantiles_kernel_shape()
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
