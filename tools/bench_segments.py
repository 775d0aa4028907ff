#!/usr/bin/env python3
"""Segment statistics on labelled clouds: per cloud one fresh child process under its own time limit, warm-up, timed repetitions with device
events, medians with their spread, one JSON line.

`--points` points of two clouds -- the uniform box (1000 m a side) and the LiDAR-like sheet of the other benches -- in ONE columnar
Position3D buffer, with three labellings drawn from a seed:
  four     4 segments, segment 0 with 94 % of the points (the ground), 2 % each for the others
  trees    points / 1000 segments of about 300 points, 70 % of the points unlabelled
  regions  points / 50 segments of about 40 points, 20 % of the points unlabelled
each in two buffer orders: `random` as drawn, and `sorted` with the points permuted so that the labels ascend.  Measured per run:
pst_segment_statistics with all eight statistics and the apex, and with COUNT | BOUNDS alone; its three phases (PST_SEGMENTS_TIMES=1,
pst_segments_phase_times) and the number of fold levels the largest segment needs.  Yardsticks in the same process on the same buffers:
pst_rasterize with all five statistics on 1 m cells (the same sort + gather + reduce with one channel), pst_calculate_bounds, and the host
loop the call replaces -- cluster_mask -> filter_into -> calculate_bounds -- for the 100 largest segments.

    python tools/bench_segments.py [--points 100000000] [--reps 3] [--warmup 1] [--limit 900] [--out profiles/segments_1e8.json]
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

NONE = 0xFFFFFFFF
LABELLINGS = ("four", "trees", "regions")
ORDERS = ("random", "sorted")
LOOP_SEGMENTS = 100


def say(text):
    print(text, file=sys.stderr, flush=True)


def make_cloud(torch, name, n, seed):
    from bench_clusters import sheet_cloud
    if name == "sheet":
        return sheet_cloud(torch, n, seed)
    if name == "uniform":
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g) * 1000.0
    sys.exit(f"unknown cloud {name!r}")


def make_labels(torch, name, n, seed):
    """(labels as int64 with -1 for none, n_segments)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    u = torch.rand(n, device="cuda", generator=g)
    if name == "four":
        labels = torch.zeros(n, dtype=torch.int64, device="cuda")
        for s, lo in ((1, 0.94), (2, 0.96), (3, 0.98)):
            labels[u >= lo] = s
        return labels, 4
    S, labelled = (max(1, n // 1000), 0.3) if name == "trees" else (max(1, n // 50), 0.8)
    labels = torch.randint(0, S, (n,), device="cuda", generator=g)
    labels[u >= labelled] = -1
    return labels, S


def levels_of(largest):
    """levels of the tree over a segment of `largest` members"""
    k, m = 1, -(-int(largest) // 256)
    while m > 1:
        m, k = -(-m // 256), k + 1
    return k


def child(args):
    """One cloud; prints its JSON object on the last line of stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_segments.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A
    from bench_clusters import quartiles, timed

    hip = pa.product_api()
    n = args.points
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    cloud = make_cloud(torch, args.child, n, 42)
    out = {}
    all_bits, few_bits = alg.segment_stats_bits(alg.SEGMENT_STATS), alg.segment_stats_bits(("count", "bounds"))
    for labelling in args.labellings.split(","):
        labels64, S = make_labels(torch, labelling, n, 7)
        counts = torch.bincount(labels64[labels64 >= 0], minlength=S)
        row = {"n_segments": S, "members": int(counts.sum()), "largest_segment": int(counts.max()), "fold_levels": levels_of(counts.max())}
        for order in ORDERS:
            if order == "sorted":
                perm = torch.argsort(torch.where(labels64 < 0, torch.full_like(labels64, S), labels64), stable=True)
                pos, lab = cloud[perm].contiguous(), labels64[perm]
                del perm
            else:
                pos, lab = cloud, labels64
            lab32 = lab.to(torch.int32)  # (-1 becomes 0xFFFFFFFF: the u32 bit pattern in an int32 tensor)
            buf = pa.ExternalColumnsBuffer([pos], layout, n)
            planes = torch.empty((alg.segment_planes(all_bits), S), dtype=torch.float64, device="cuda")
            apex = torch.empty(S, dtype=torch.int32, device="cuda")
            members = C.c_uint64()

            def call(bits, with_apex):
                hip.segment_statistics(buf._h, C.c_void_p(lab32.data_ptr()), S, None, None, bits, C.c_void_p(planes.data_ptr()),
                                       C.c_void_p(apex.data_ptr()) if with_apex else None, 0, C.byref(members))
            call(all_bits, True)  # (untimed: the library must see the cloud torch made before anything is measured on it)
            if members.value != row["members"] or not torch.equal(planes[0], counts.to(torch.float64)):
                sys.exit(f"{labelling} {order}: the counts are not the labels' counts")
            t_all, phases = timed(torch, lambda: call(all_bits, True), args.warmup, args.reps, after=lambda: alg.segments_phase_times(hip))
            p = np.median(np.asarray(phases), axis=0)
            t_few = timed(torch, lambda: call(few_bits, False), args.warmup, args.reps)[0]
            run = {"all_statistics": quartiles(t_all), "count_and_bounds": quartiles(t_few),
                   "phases_ms": {"keys_sort_directory": round(float(p[0]), 4), "gather": round(float(p[1]), 4), "folds_and_output": round(float(p[2]), 4)}}
            # the yardsticks on the same buffer
            grid = alg.pmf_grid(buf, 1.0)
            raster = torch.empty((5, grid["rows"], grid["cols"]), dtype=torch.float64, device="cuda")
            t_raster = quartiles(timed(torch, lambda: alg.rasterize(buf, 1.0, ("count", "min", "max", "mean", "variance"), device_out_ptr=raster.data_ptr()), args.warmup, args.reps)[0])
            t_bounds = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
            del raster
            largest = torch.argsort(counts, descending=True, stable=True)[:LOOP_SEGMENTS]
            largest, sizes = largest.tolist(), counts[largest].tolist()
            mask = torch.empty(n, dtype=torch.uint8, device="cuda")

            def loop():
                for s, size in zip(largest, sizes):
                    alg.cluster_mask(lab32.data_ptr(), n, s, 1, mask.data_ptr(), api=hip)
                    one = pa.HashMapBuffer.new_from_layout(layout)
                    one.resize(size)
                    buf.filter_into(one, (mask.data_ptr(), "device"), size)
                    alg.calculate_bounds(one)
            t_loop = quartiles(timed(torch, loop, 0, 1)[0])
            run["yardsticks"] = {"rasterize_all_five": t_raster, "calculate_bounds": t_bounds, "host_loop": dict(t_loop, segments=len(largest))}
            run["ratios"] = {"all_to_rasterize": round(run["all_statistics"]["median_ms"] / t_raster["median_ms"], 3),
                             "count_and_bounds_to_calculate_bounds": round(run["count_and_bounds"]["median_ms"] / t_bounds["median_ms"], 3),
                             "all_to_host_loop": round(run["all_statistics"]["median_ms"] / t_loop["median_ms"], 4),
                             "host_loop_per_segment_ms": round(t_loop["median_ms"] / max(1, len(largest)), 4)}
            row[order] = run
            say(f"  {args.child} {labelling} {order}: {run}")
            del buf, planes, apex, mask, lab32
            if order == "sorted":
                del pos, lab
        out[labelling] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clouds", default="uniform,sheet")
    ap.add_argument("--labellings", default=",".join(LABELLINGS))
    ap.add_argument("--limit", type=int, default=900, help="seconds one child process may take; after a child that fails or runs out of time no other is started")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    result = {"bench": "segments", "points": args.points, "seed": 42, "loop_segments": LOOP_SEGMENTS}
    base = [sys.executable, os.path.abspath(__file__), "--points", str(args.points), "--reps", str(args.reps), "--warmup", str(args.warmup), "--labellings", args.labellings]
    ok = True
    for name in args.clouds.split(","):
        if not ok:
            result[name] = {"skipped": "an earlier cloud failed or ran out of time"}
            continue
        say(name)
        try:
            r = subprocess.run(base + ["--child", name], env=dict(os.environ, PST_SEGMENTS_TIMES="1"), stdout=subprocess.PIPE, text=True, timeout=args.limit)
            ok = r.returncode == 0
            result[name] = json.loads(r.stdout.strip().splitlines()[-1]) if ok else {"failed": r.returncode}
        except subprocess.TimeoutExpired:
            ok = False
            result[name] = {"failed": f"no result within {args.limit} s"}
    try:
        import pasture_amd as pa
        result["kernel_shape"] = pa.segments_kernel_shape()
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
