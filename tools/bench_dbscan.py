#!/usr/bin/env python3
"""DBSCAN on synthetic points: one fresh process, warm-up, timed repetitions with device events, medians, one JSON line.

Two clouds of the same size, each in ONE columnar Position3D buffer:
  uniform   synth_fill points in the bench's box
  sheet     the LiDAR-like sheet of bench.py's kNN leg (a noisy 2-D manifold with 0.001 % far strays)
eps comes from the density, so that a point has about 8 others within it (a ball for the box, a disc for the sheet); the mean that results is
measured on 4096 sampled points and reported.  pst_dbscan runs with min_points 1, 4 and 16: every point core, most points core, few points
core.  Comparisons in the same process on the same buffer: pst_euclidean_clusters at the same radius (the yardstick: DBSCAN builds the same
index and walks the same cells), pst_radius_outlier_mask with 8 neighbours at the same radius, and pst_calculate_bounds (one pass over the
positions).  The split of a call between index build, core count, link and border + bookkeeping comes from stream events inside the call
(PST_DBSCAN_TIMES=1, pst_dbscan_phase_times).

    python tools/bench_dbscan.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/dbscan_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_DBSCAN_TIMES"] = "1"  # read once, at the library's first DBSCAN call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms, dtype=np.float64), [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "min_ms": round(float(min(ms)), 4), "reps": len(ms)}


def timed(torch, fn, warmup, reps, after=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out, extra = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
        if after:
            extra.append(after())
    return out, extra


def sheet_cloud(torch, n, seed):
    """bench.py's _sheet_cloud"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    xy = torch.rand(n, 2, device="cuda", dtype=torch.float64, generator=g) * 1000.0
    z = 10.0 * torch.sin(xy[:, 0] / 50.0) * torch.cos(xy[:, 1] / 80.0) + 50.0 + 0.02 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g)
    sheet = torch.cat([xy, z[:, None]], dim=1).contiguous()
    n_stray = max(1, n // 100000)
    sheet[torch.randint(0, n, (n_stray,), device="cuda", generator=g), 2] = (torch.rand(n_stray, device="cuda", dtype=torch.float64, generator=g) - 0.5) * 6000.0
    return sheet


MIN_POINTS = (1, 4, 16)


def measure(torch, pa, alg, hip, buf, n, eps, args):
    """One cloud: the DBSCAN call at every min_points with its phases, the three yardsticks, the measured neighbour count."""
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    core = torch.empty(n, dtype=torch.uint8, device="cuda")
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    counts = (C.c_uint64 * 3)()
    count, clustered, kept = C.c_uint64(), C.c_uint64(), C.c_uint64()
    out = {"eps": eps}

    def clusters():
        hip.euclidean_clusters(buf._h, eps, 1, 2 ** 64 - 1, C.c_void_p(labels.data_ptr()), 0, None, 0, C.byref(count), C.byref(clustered))

    t_clusters = quartiles(timed(torch, clusters, args.warmup, args.reps)[0])
    for min_points in MIN_POINTS:
        def dbscan():
            hip.dbscan(buf._h, eps, min_points, C.c_void_p(labels.data_ptr()), C.c_void_p(core.data_ptr()), 0, None, 0, counts)

        t_call, phases = timed(torch, dbscan, args.warmup, args.reps, after=lambda: alg.dbscan_phase_times(hip))
        t_call = quartiles(t_call)
        phases = np.median(np.asarray(phases), axis=0)
        out[f"min_points_{min_points}"] = {
            "clusters": int(counts[0]), "core_points": int(counts[1]), "border_points": int(counts[2] - counts[1]), "noise_points": int(n - counts[2]),
            "call": t_call,
            "phases_ms": {"index_build": round(float(phases[0]), 4), "core_count": round(float(phases[1]), 4), "link": round(float(phases[2]), 4),
                          "border_and_bookkeeping": round(float(phases[3]), 4)},
            "ratio_to_euclidean_clusters": round(t_call["median_ms"] / t_clusters["median_ms"], 4)}
    t_radius = quartiles(timed(torch, lambda: hip.radius_outlier_mask(buf._h, eps, 8, C.c_void_p(mask.data_ptr()), 0, C.byref(kept)), args.warmup, args.reps)[0])
    t_bounds = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    # how many others a point really has within eps: 4096 sampled rows of a 17-neighbour search (so the count saturates at 16)
    k = 17
    dist = torch.empty(n * k, dtype=torch.float64, device="cuda")
    alg.knn_search_device(buf, k, dist.data_ptr())
    rows = torch.randint(0, n, (4096,), device="cuda")
    d2 = dist.view(n, k)[rows, 1:]
    within = float(((d2 * d2) <= eps * eps).sum(dim=1).double().mean())
    del dist
    out.update({"mean_neighbours_within_eps": round(within, 3), "neighbour_count_saturates_at": k - 1,
                "euclidean_clusters": dict(t_clusters, clusters=int(count.value)), "radius_outlier_mask_8": t_radius, "calculate_bounds": t_bounds})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--neighbours", type=float, default=8.0, help="others a point should have within eps, from the density")
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dbscan.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    result = {"bench": "dbscan", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.dbscan_kernel_shape(hip),
              "neighbours_aimed_at": args.neighbours}
    for name in args.clouds.split(","):
        if name == "uniform":
            buf = pa.HashMapBuffer.new_from_layout(layout)
            buf.resize(n)
            buf.synth_fill(42, 0)
            b = alg.calculate_bounds(buf)
            volume = float(np.prod(np.asarray(b.max()) - np.asarray(b.min())))
            eps = (args.neighbours / (4.0 / 3.0 * math.pi * n / volume)) ** (1.0 / 3.0)  # a ball that holds `neighbours` points on average
            result[name] = measure(torch, pa, alg, hip, buf, n, eps, args)
        elif name == "sheet":
            sheet = sheet_cloud(torch, n, 42)
            buf = pa.ExternalColumnsBuffer([sheet], layout, n)
            eps = math.sqrt(args.neighbours / (math.pi * n / 1.0e6))  # a disc on the 1000 x 1000 sheet
            result[name] = measure(torch, pa, alg, hip, buf, n, eps, args)
            del sheet
        else:
            sys.exit(f"unknown cloud {name!r}")
        del buf
        hip.release_scratch()
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
