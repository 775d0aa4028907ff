#!/usr/bin/env python3
"""Geometric features on synthetic points: one fresh process, warm-up, timed repetitions with device events, median and IQR, one JSON line.

Two clouds (a uniform box of synth_fill points; the LiDAR-like sheet of bench.py's kNN leg), k = 10 and 16.  Per cloud and k, all in the same
run on the same buffer:
  full          pst_geometric_features, linearity + planarity + scattering + verticality: the search, then the kernel
  kernel        pst_geometric_features_from_knn_device alone on the lists the full call returned (four planes; and all thirteen with both vectors)
  knn_search    pst_knn_search_device (lists and distances)
  normals       pst_compute_normals_device (normals and curvature): what the library could say about a neighbourhood before
  bounds        pst_calculate_bounds: one streaming pass over the positions, the floor of anything that reads them
ratio_kernel_to_search = kernel / (full - kernel): the expectation to confirm or refute is that the feature kernel costs less than the search
it follows.

    python tools/bench_features.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/features_1e8.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = 8 | 16 | 32 | 512  # linearity, planarity, scattering, verticality


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
    return quartiles(out)


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


def measure(torch, alg, hip, buf, n, k, args):
    inf = float("inf")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    knn = torch.empty(n * k, dtype=torch.int32, device="cuda")
    out = torch.empty(13 * n, dtype=torch.float64, device="cuda")
    vec = torch.empty(2 * 3 * n, dtype=torch.float64, device="cuda")
    normals, directions = vec[:3 * n], vec[3 * n:]
    t_full = timed(torch, lambda: hip.geometric_features(buf._h, k, inf, DEFAULT, p(out), None, None, p(knn)), args.warmup, args.reps)

    def kernel(features, nr, dr):  # (the entry is stream-ordered: the wait is part of the repetition, as it is of the synchronous calls)
        hip.geometric_features_from_knn_device(buf._h, k, p(knn), inf, features, p(out), nr, dr)
        hip.stream_synchronize()

    t_kernel = timed(torch, lambda: kernel(DEFAULT, None, None), args.warmup, args.reps)
    t_all = timed(torch, lambda: kernel(8191, p(normals), p(directions)), args.warmup, args.reps)
    planes = out.view(13, n)
    means = {name: round(float(torch.nanmean(planes[t])), 6) for name, t in (("linearity", 3), ("planarity", 4), ("scattering", 5), ("verticality", 9), ("count", 12))}
    del out
    dist = torch.empty(n * k, dtype=torch.float64, device="cuda")
    t_search = timed(torch, lambda: hip.knn_search_device(buf._h, k, p(knn), p(dist)), args.warmup, args.reps)
    del dist
    curvature = torch.empty(n, dtype=torch.float64, device="cuda")
    t_normals = timed(torch, lambda: hip.compute_normals_device(buf._h, k, p(normals), p(curvature), None), args.warmup, args.reps)
    t_bounds = timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)
    search_in_full = t_full["median_ms"] - t_kernel["median_ms"]
    return {"k": k, "points_per_block": alg.features_kernel_shape(k, hip)["points_per_block"], "full": t_full, "kernel": t_kernel, "kernel_all_planes_and_vectors": t_all,
            "knn_search_device": t_search, "compute_normals_device": t_normals, "calculate_bounds": t_bounds, "search_in_full_ms": round(search_in_full, 4),
            "ratio_kernel_to_search": round(t_kernel["median_ms"] / search_in_full, 4), "kernel_costs_less_than_search": bool(t_kernel["median_ms"] < search_in_full),
            "ratio_full_to_knn_search_device": round(t_full["median_ms"] / t_search["median_ms"], 4),
            "ratio_full_to_compute_normals_device": round(t_full["median_ms"] / t_normals["median_ms"], 4),
            "kernel_ns_per_point": round(t_kernel["median_ms"] * 1e6 / n, 4), "mean_of_planes": means}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", default="10,16")
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_features.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    result = {"bench": "features", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "features_of_full_and_kernel": ["linearity", "planarity", "scattering", "verticality"]}
    for name in args.clouds.split(","):
        if name == "uniform":
            buf = pa.HashMapBuffer.new_from_layout(layout)
            buf.resize(n)
            buf.synth_fill(42, 0)
            held = None
        elif name == "sheet":
            held = sheet_cloud(torch, n, 42)
            buf = pa.ExternalColumnsBuffer([held], layout, n)
        else:
            sys.exit(f"unknown cloud {name!r}")
        result[name] = [measure(torch, alg, hip, buf, n, int(k), args) for k in args.k.split(",")]
        del buf, held
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
