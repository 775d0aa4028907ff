#!/usr/bin/env python3
"""Outlier masks on synthetic points: one fresh process, warm-up, timed repetitions with device events, median and IQR, one JSON line.

Three calls on ONE columnar Position3D buffer of synth_fill points:
  statistical   pst_statistical_outlier_mask, mean_k = 16 (the search runs with k = 17), device mask
  radius        pst_radius_outlier_mask, min_neighbours = 8 (k = 9), device mask
  search        pst_compute_normals_device with only the neighbour lists requested, at k = 17 and at k = 9: the search both masks are built on, and
                all the library could do before them -- the yardstick.  ratio = mask call / search at the same k.

    python tools/bench_outliers.py [--points 100000000] [--reps 10] [--warmup 2] [--out profiles/outliers_1e8.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms, dtype=np.float64), [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(ms)), 4), "reps": len(ms)}


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mean-k", type=int, default=16)
    ap.add_argument("--stddev-mult", type=float, default=1.0)
    ap.add_argument("--min-neighbours", type=int, default=8)
    ap.add_argument("--radius", type=float, default=None, help="default: the median distance to the min_neighbours-th neighbour over 4096 sampled points")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_outliers.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    buf = pa.HashMapBuffer.new_from_layout(pa.PointLayout.from_attributes([A.POSITION_3D], api=hip))
    buf.resize(n)
    buf.synth_fill(42, 0)
    k_stat, k_rad = max(args.mean_k + 1, 3), max(args.min_neighbours + 1, 3)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    knn = torch.empty(n * max(k_stat, k_rad), dtype=torch.int32, device="cuda")
    stats, kept = (C.c_double * 4)(), C.c_uint64()

    def search(k):
        return lambda: hip.compute_normals_device(buf._h, k, None, None, C.c_void_p(knn.data_ptr()))

    radius = args.radius
    if radius is None:  # about half of the points have min_neighbours others this close
        dist = torch.empty(n * k_rad, dtype=torch.float64, device="cuda")
        alg.knn_search_device(buf, k_rad, dist.data_ptr())
        rows = torch.randint(0, n, (4096,), device="cuda")
        radius = float(dist.view(n, k_rad)[rows, args.min_neighbours].median())
        del dist

    t_search_stat = quartiles(timed(torch, search(k_stat), args.warmup, args.reps))
    t_search_rad = quartiles(timed(torch, search(k_rad), args.warmup, args.reps))
    t_stat = quartiles(timed(torch, lambda: hip.statistical_outlier_mask(buf._h, args.mean_k, args.stddev_mult, C.c_void_p(mask.data_ptr()), 0, None, stats, C.byref(kept)),
                             args.warmup, args.reps))
    stat_result = {"mean": stats[0], "stddev": stats[1], "threshold": stats[2], "count": int(stats[3]), "kept": kept.value}
    t_rad = quartiles(timed(torch, lambda: hip.radius_outlier_mask(buf._h, radius, args.min_neighbours, C.c_void_p(mask.data_ptr()), 0, C.byref(kept)), args.warmup, args.reps))
    result = {"bench": "outliers", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.outlier_kernel_shape(hip),
              "statistical": {"mean_k": args.mean_k, "k_search": k_stat, "stddev_mult": args.stddev_mult, "call": t_stat, "search_only": t_search_stat,
                              "ratio": round(t_stat["median_ms"] / t_search_stat["median_ms"], 4),
                              "added_ms": round(t_stat["median_ms"] - t_search_stat["median_ms"], 4), "result": stat_result},
              "radius": {"min_neighbours": args.min_neighbours, "k_search": k_rad, "radius": radius, "call": t_rad, "search_only": t_search_rad,
                         "ratio": round(t_rad["median_ms"] / t_search_rad["median_ms"], 4),
                         "added_ms": round(t_rad["median_ms"] - t_search_rad["median_ms"], 4), "kept": kept.value}}
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
