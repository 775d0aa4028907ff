#!/usr/bin/env python3
"""Minimum-distance (Poisson-disk) subsampling on synthetic points: one fresh process, warm-up, timed repetitions with device events, medians,
one JSON line.

Two clouds of the same size, each in ONE columnar Position3D buffer:
  uniform   synth_fill points in the bench's box
  sheet     the LiDAR-like sheet of bench.py's kNN leg (a noisy 2-D manifold with 0.001 % far strays)
The radius comes from the density as tools/bench_clusters.py chooses its tolerance, so that a point has about 8 others within it.  Per cloud
the shuffled call is timed; its three phases come from stream events inside the call (PST_SAMPLE_TIMES=1, pst_sample_phase_times), `rounds`
from the call itself.  Yardsticks in the same process on the same buffer: pst_euclidean_clusters at tolerance = radius (it builds the same
index) and pst_calculate_bounds (one pass over the positions).
Index order needs a round per link of the longest chain of conflicts, hundreds of rounds on ordered input (include/pasture_amd.h), so its two
legs -- the sheet as generated (shuffled input) and the same sheet sorted into scan lines -- run on the first --index-points points of the sheet
at the radius that matches THAT density, once each, and are reported with that size.  The C ABI reports the number of rounds, not the active
count of each: that column is not recorded.

    python tools/bench_sample.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/sample_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_SAMPLE_TIMES"] = "1"  # read once, at the library's first subsampling call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clusters import quartiles, sheet_cloud, timed  # noqa: E402


def sample_leg(torch, alg, hip, buf, n, radius, order, seed, warmup, reps):
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    kept, rounds = C.c_uint64(), C.c_uint32()

    def call():
        hip.poisson_disk_mask(buf._h, radius, order, seed, C.c_void_p(mask.data_ptr()), 0, C.byref(kept), C.byref(rounds))

    t_call, phases = timed(torch, call, warmup, reps, after=lambda: alg.sample_phase_times(hip))
    phases = np.median(np.asarray(phases), axis=0)
    return {"order": "shuffled" if order == 0 else "index", "points": n, "radius": radius, "kept": int(kept.value), "rounds": int(rounds.value), "call": quartiles(t_call),
            "phases_ms": {"index_build": round(float(phases[0]), 4), "decision_rounds": round(float(phases[1]), 4), "mask_write": round(float(phases[2]), 4)}}


def measure(torch, alg, hip, buf, n, radius, args):
    """One cloud: the shuffled call with its phases and the two yardsticks."""
    out = sample_leg(torch, alg, hip, buf, n, radius, 0, 42, args.warmup, args.reps)
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    count, clustered = C.c_uint64(), C.c_uint64()

    def clusters():
        hip.euclidean_clusters(buf._h, radius, 1, 2 ** 64 - 1, C.c_void_p(labels.data_ptr()), 0, None, 0, C.byref(count), C.byref(clustered))

    t_clusters = quartiles(timed(torch, clusters, args.warmup, args.reps)[0])
    t_bounds = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    out.update({"euclidean_clusters_at_radius": t_clusters, "calculate_bounds": t_bounds,
                "ratio_to_euclidean_clusters": round(out["call"]["median_ms"] / t_clusters["median_ms"], 4),
                "ratio_to_calculate_bounds": round(out["call"]["median_ms"] / t_bounds["median_ms"], 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--index-points", type=int, default=1_000_000, help="points of the two index-order legs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--neighbours", type=float, default=8.0, help="others a point should have within the radius, from the density")
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sample.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    result = {"bench": "sample", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.sample_kernel_shape(hip),
              "neighbours_aimed_at": args.neighbours}
    for name in args.clouds.split(","):
        if name == "uniform":
            buf = pa.HashMapBuffer.new_from_layout(layout)
            buf.resize(n)
            buf.synth_fill(42, 0)
            b = alg.calculate_bounds(buf)
            volume = float(np.prod(np.asarray(b.max()) - np.asarray(b.min())))
            radius = (args.neighbours / (4.0 / 3.0 * math.pi * n / volume)) ** (1.0 / 3.0)  # a ball that holds `neighbours` points on average
            result[name] = measure(torch, alg, hip, buf, n, radius, args)
        elif name == "sheet":
            sheet = sheet_cloud(torch, n, 42)
            buf = pa.ExternalColumnsBuffer([sheet], layout, n)
            radius = math.sqrt(args.neighbours / (math.pi * n / 1.0e6))  # a disc on the 1000 x 1000 sheet
            result[name] = measure(torch, alg, hip, buf, n, radius, args)
            # index order: a prefix of the sheet (the same 1000 x 1000 extent, thinner), as generated and sorted into scan lines 4 radii wide
            m = min(args.index_points, n)
            r_m = math.sqrt(args.neighbours / (math.pi * m / 1.0e6))
            part = sheet[:m].contiguous()
            result["sheet_index_order_shuffled_input"] = sample_leg(torch, alg, hip, pa.ExternalColumnsBuffer([part], layout, m), m, r_m, 1, 0, 0, 1)
            line = torch.floor(part[:, 1] / (4.0 * r_m))
            lines = part[torch.argsort(line * 2048.0 + part[:, 0])].contiguous()  # (x < 1000: the line number decides first)
            result["sheet_index_order_scan_line_input"] = sample_leg(torch, alg, hip, pa.ExternalColumnsBuffer([lines], layout, m), m, r_m, 1, 0, 0, 1)
            result["sheet_shuffled_order_scan_line_input"] = sample_leg(torch, alg, hip, pa.ExternalColumnsBuffer([lines], layout, m), m, r_m, 0, 42, 0, 1)
            del sheet, part, lines
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
