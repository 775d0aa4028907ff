#!/usr/bin/env python3
"""RANSAC plane / line fit on synthetic points: one fresh process, warm-up, timed repetitions with device events, median and IQR, one JSON line.

Legs: columnar Position3D (24 B per point), interleaved Position3D alone (24-byte records) and the typed LAS format 0 record (35 bytes); plane and
line; 32 and 300 iterations; threshold 0.5.  Per leg: ms per *_fit call (table + scoring + arg-max + the copies of the result), ms per inlier
mask pass, point-hypothesis pairs per second, and -- in the same run on the same buffer -- the time of pst_calculate_bounds, one clean pass over the
same bytes: a design that streamed the cloud once per hypothesis could not beat iterations x that time.

    python tools/bench_ransac.py [--points 100000000] [--reps 20] [--warmup 3] [--out profiles/ransac_fit_1e8.json]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, nargs="*", default=[32, 300])
    ap.add_argument("--layouts", nargs="*", default=["columnar24", "interleaved24", "interleaved35"])
    ap.add_argument("--models", nargs="*", default=["plane", "line"])
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--only-fit", action="store_true", help="one leg's fit calls and nothing else (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ransac.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg, las
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    shape = alg.ransac_kernel_shape(hip)
    legs = []
    for layout_name in args.layouts:
        if layout_name == "interleaved35":
            layout, kind = las.point_layout_from_las_point_format(las.Format(0), False, api=hip), pa.VectorBuffer
        else:
            layout, kind = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip), pa.HashMapBuffer if layout_name == "columnar24" else pa.VectorBuffer
        buf = kind.new_from_layout(layout)
        buf.resize(n)
        buf.synth_fill(42, 0)
        bytes_per_point = 24 if layout_name == "columnar24" else layout.size_of_point_entry()
        mask = torch.empty(n, dtype=torch.uint8, device="cuda")
        mn, mx, has = (C.c_double * 3)(), (C.c_double * 3)(), C.c_int()
        t_bounds = None
        if not args.only_fit:
            t_bounds = quartiles(timed(torch, lambda: hip.calculate_bounds(buf._h, mn, mx, C.byref(has)), args.warmup, args.reps))
        for model_name in args.models:
            line = model_name == "line"
            per = 2 if line else 3
            fit = hip.ransac_line_fit if line else hip.ransac_plane_fit
            mask_fn = hip.line_inlier_mask_device if line else hip.plane_inlier_mask_device
            for iterations in args.iterations:
                samples = alg.ransac_sample_indices(7, n, iterations, per, api=hip)
                model, ranking, best = (C.c_double * 6)(), C.c_uint64(), C.c_size_t()
                sp = samples.ctypes.data_as(C.POINTER(C.c_uint64))

                def run_fit():
                    fit(buf._h, args.threshold, sp, iterations, model, C.byref(ranking), C.byref(best), None)

                t_fit = quartiles(timed(torch, run_fit, args.warmup, args.reps))
                leg = {"layout": layout_name, "bytes_per_point": bytes_per_point, "model": model_name, "iterations": iterations, "fit": t_fit,
                       "ranking": ranking.value, "best_iteration": best.value,
                       "pairs_per_s": round(n * iterations / (t_fit["median_ms"] * 1e-3), 1),
                       "passes_over_positions": -(-iterations // shape["batch"])}
                if not args.only_fit:
                    def run_mask():
                        mask_fn(buf._h, model, args.threshold, C.c_void_p(mask.data_ptr()))
                        hip.stream_synchronize()

                    leg["mask"] = quartiles(timed(torch, run_mask, args.warmup, args.reps))
                    leg["bounds"] = t_bounds
                    leg["iterations_x_bounds_ms"] = round(iterations * t_bounds["median_ms"], 3)
                    leg["fit_over_iterations_x_bounds"] = round(t_fit["median_ms"] / (iterations * t_bounds["median_ms"]), 4)
                legs.append(leg)
        del buf, mask
        alg.release_scratch(hip)
    result = {"bench": "ransac_fit", "points": n, "threshold": args.threshold, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": shape,
              "legs": legs}
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
