#!/usr/bin/env python3
"""Region growing on synthetic points: one fresh process, warm-up, timed repetitions with device events, medians, one JSON line.

Two clouds of the same size, each in ONE columnar Position3D buffer:
  uniform   synth_fill points in the bench's box (no surface anywhere: nearly every point is a rim point or alone)
  sheet     the LiDAR-like sheet of bench.py's kNN leg (a noisy 2-D manifold with 0.001 % far strays: one region holds most of the cloud)
At k = 10 and 16: pst_region_growing (search, features, regions) with its three phases from stream events inside the call
(PST_REGION_TIMES=1, pst_region_phase_times), and pst_region_growing_from_knn alone on the lists, normals and curvature the call handed back,
with its phases.  Comparisons in the same process on the same buffer: pst_geometric_features at the same k (the search and the feature kernel
the full call starts with), the feature kernel alone on the same lists (link does the same gathers with less arithmetic), pst_dbscan at a
radius that holds about 8 others (its border + bookkeeping phase is what attach + numbering is to be compared with), and pst_calculate_bounds
(one pass over the positions).

    python tools/bench_region.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/region_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_REGION_TIMES"] = "1"  # read once, at the library's first call of either kind
os.environ["PST_DBSCAN_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_dbscan import quartiles, sheet_cloud, timed  # noqa: E402

KS = (10, 16)
SURFACE_VARIATION = 128


def phases_of(samples):
    p = np.median(np.asarray(samples), axis=0)
    return {"search_and_features": round(float(p[0]), 4), "classify_and_link": round(float(p[1]), 4), "attach_and_numbering": round(float(p[2]), 4)}


def measure(torch, alg, hip, buf, n, eps, args):
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    smooth = torch.empty(n, dtype=torch.uint8, device="cuda")
    normals = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    curvature = torch.empty(n, dtype=torch.float64, device="cuda")
    counts = (C.c_uint64 * 3)()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cos, inf = math.cos(math.radians(args.smoothness_deg)), float("inf")
    out = {"min_abs_cos": cos, "curvature_threshold": args.curvature_threshold}
    for k in KS:
        knn = torch.empty(n * k, dtype=torch.int32, device="cuda")

        def full():
            hip.region_growing(buf._h, k, cos, args.curvature_threshold, inf, 1, 2 ** 64 - 1, p(labels), p(smooth), 0, None, 0, counts, p(normals), p(curvature), p(knn))

        def from_lists():
            hip.region_growing_from_knn(buf._h, k, p(knn), p(normals), p(curvature), cos, args.curvature_threshold, inf, 1, 2 ** 64 - 1, p(labels), p(smooth), 0, None, 0,
                                        counts)

        def features():
            hip.geometric_features(buf._h, k, inf, SURFACE_VARIATION, p(curvature), p(normals), None, p(knn))

        def feature_kernel():
            hip.geometric_features_from_knn_device(buf._h, k, p(knn), inf, SURFACE_VARIATION, p(curvature), p(normals), None)
            hip.stream_synchronize()

        t_full, ph_full = timed(torch, full, args.warmup, args.reps, after=lambda: alg.region_phase_times(hip))
        found = {"regions": int(counts[0]), "smooth_points": int(counts[1]), "rim_points_labelled": None, "labelled_points": int(counts[2])}
        t_lists, ph_lists = timed(torch, from_lists, args.warmup, args.reps, after=lambda: alg.region_phase_times(hip))
        assert (int(counts[0]), int(counts[1]), int(counts[2])) == (found["regions"], found["smooth_points"], found["labelled_points"])
        sm = int(smooth.sum(dtype=torch.int64))
        found["rim_points_labelled"] = int((labels != -1).sum()) - int(((labels != -1) & (smooth != 0)).sum())
        assert sm == found["smooth_points"]
        t_features = quartiles(timed(torch, features, args.warmup, args.reps)[0])
        t_kernel = quartiles(timed(torch, feature_kernel, args.warmup, args.reps)[0])
        t_full, t_lists = quartiles(t_full), quartiles(t_lists)
        ph_full, ph_lists = phases_of(ph_full), phases_of(ph_lists)
        out[f"k_{k}"] = dict(found, kernel_shape=alg.region_kernel_shape(k, hip), call=t_full, phases_ms=ph_full, from_lists=t_lists, from_lists_phases_ms=ph_lists,
                             geometric_features=t_features, feature_kernel_alone=t_kernel,
                             ratio_to_geometric_features=round(t_full["median_ms"] / t_features["median_ms"], 4),
                             link_to_feature_kernel=round(ph_lists["classify_and_link"] / t_kernel["median_ms"], 4))
        del knn
    core = torch.empty(n, dtype=torch.uint8, device="cuda")

    def dbscan():
        hip.dbscan(buf._h, eps, 4, p(labels), p(core), 0, None, 0, counts)

    t_dbscan, ph = timed(torch, dbscan, args.warmup, args.reps, after=lambda: alg.dbscan_phase_times(hip))
    ph = np.median(np.asarray(ph), axis=0)
    out["dbscan_min_points_4"] = dict(quartiles(t_dbscan), eps=eps, clusters=int(counts[0]), border_and_bookkeeping_ms=round(float(ph[3]), 4))
    for k in KS:
        out[f"k_{k}"]["attach_and_numbering_to_dbscan_border"] = round(out[f"k_{k}"]["from_lists_phases_ms"]["attach_and_numbering"] / float(ph[3]), 4)
    out["calculate_bounds"] = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--smoothness-deg", type=float, default=10.0)
    ap.add_argument("--curvature-threshold", type=float, default=0.02)
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_region.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    result = {"bench": "region_growing", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "smoothness_deg": args.smoothness_deg}
    for name in args.clouds.split(","):
        if name == "uniform":
            buf = pa.HashMapBuffer.new_from_layout(layout)
            buf.resize(n)
            buf.synth_fill(42, 0)
            b = alg.calculate_bounds(buf)
            volume = float(np.prod(np.asarray(b.max()) - np.asarray(b.min())))
            eps = (8.0 / (4.0 / 3.0 * math.pi * n / volume)) ** (1.0 / 3.0)  # a ball that holds 8 points on average
            result[name] = measure(torch, alg, hip, buf, n, eps, args)
        elif name == "sheet":
            sheet = sheet_cloud(torch, n, 42)
            buf = pa.ExternalColumnsBuffer([sheet], layout, n)
            eps = math.sqrt(8.0 / (math.pi * n / 1.0e6))  # a disc on the 1000 x 1000 sheet
            result[name] = measure(torch, alg, hip, buf, n, eps, args)
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
