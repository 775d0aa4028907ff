#!/usr/bin/env python3
"""Gather by index and the device sort orders on synthetic points: one fresh process, warm-up, timed repetitions with device events, medians,
one JSON line.

Gather legs, for Position3D-only points (24 B) and typed LAS-0 points, columnar and interleaved (source and target of the same kind): the
stream-ordered gather by the identity, by a random permutation and by the cloud's own Morton order, u32 indices in device memory.  Next to
them, on the same buffers: pst_buffer_filter_into_async with an all-ones mask -- the compaction moves the same bytes with no indirection, the
yardstick of the identity gather; it is defined on columnar sources only -- and pst_calculate_bounds (one pass over the positions).
Sort-order legs on a columnar {Position3D, Intensity, GpsTime} cloud: u16 Intensity, f64 GpsTime, z, Morton 3 x 21, each with the phase
split of pst_reorder_phase_times (PST_REORDER_TIMES=1).
Follow-on legs on the LiDAR-like sheet of bench.py's kNN leg: compute_normals_device on the shuffled cloud against the same cloud
Morton-sorted (--follow-points), and poisson_disk_mask in index order on a scan-line ordered sheet before and after shuffle (--index-points).

    python tools/bench_reorder.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/reorder_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_REORDER_TIMES"] = "1"  # read once, at the library's first reorder call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clusters import quartiles, sheet_cloud, timed  # noqa: E402


def gather_legs(torch, pa, alg, hip, layout, kind, n, args):
    src, dst = kind.new_from_layout(layout), kind.new_from_layout(layout)
    src.resize(n)
    src.synth_fill(42, 0)
    dst.resize(n)
    size = sum(a.size() for a in layout.attributes())
    out = {"points": n, "attribute_bytes_per_point": size, "record_bytes": layout.size_of_point_entry()}
    orders = {"identity": torch.arange(n, dtype=torch.int32, device="cuda"), "random_permutation": torch.randperm(n, device="cuda").to(torch.int32)}
    morton = torch.empty(n, dtype=torch.int32, device="cuda")
    alg.morton_order(src, 3, 0, device_order_ptr=morton.data_ptr())
    orders["morton_order"] = morton
    for name, idx in orders.items():
        def call():
            src.gather_into_async(dst, (idx.data_ptr(), n, 32))
            hip.stream_synchronize()
        q = quartiles(timed(torch, call, args.warmup, args.reps)[0])
        q["GB_per_s_wanted_bytes"] = round((2 * size + 4) * n / q["median_ms"] / 1e6, 1)
        out[name] = q
    del orders, morton
    if src.as_columnar() is not None:
        ones = torch.ones(n, dtype=torch.uint8, device="cuda")

        def compaction():
            src.filter_into_async(dst, ones.data_ptr(), n)
            hip.stream_synchronize()
        out["filter_into_all_ones"] = quartiles(timed(torch, compaction, args.warmup, args.reps)[0])
        out["identity_to_compaction"] = round(out["identity"]["median_ms"] / out["filter_into_all_ones"]["median_ms"], 4)
    out["calculate_bounds"] = quartiles(timed(torch, lambda: alg.calculate_bounds(src), args.warmup, args.reps)[0])
    out["random_to_identity"] = round(out["random_permutation"]["median_ms"] / out["identity"]["median_ms"], 4)
    out["morton_to_identity"] = round(out["morton_order"]["median_ms"] / out["identity"]["median_ms"], 4)
    return out


def order_legs(torch, pa, alg, hip, n, args):
    from pasture_amd.layout import attributes as A
    layout = pa.PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY, A.GPS_TIME], api=hip)
    buf = pa.HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    buf.synth_fill(42, 0)
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    legs = {"intensity_u16": lambda: alg.argsort_attribute(buf, A.INTENSITY, device_order_ptr=order.data_ptr()),
            "gps_time_f64": lambda: alg.argsort_attribute(buf, A.GPS_TIME, device_order_ptr=order.data_ptr()),
            "z_f64": lambda: alg.argsort_attribute(buf, A.POSITION_3D, 2, device_order_ptr=order.data_ptr()),
            "morton_3x21": lambda: alg.morton_order(buf, 3, 21, device_order_ptr=order.data_ptr())}
    out = {"points": n}
    for name, call in legs.items():
        t, phases = timed(torch, call, args.warmup, args.reps, after=lambda: alg.reorder_phase_times(hip))
        phases = np.median(np.asarray(phases), axis=0)
        out[name] = quartiles(t)
        out[name]["phases_ms"] = {"bounds_and_keys": round(float(phases[0]), 4), "sort": round(float(phases[1]), 4), "gather": round(float(phases[2]), 4)}
    return out


def follow_on_legs(torch, pa, alg, hip, args):
    from pasture_amd.layout import attributes as A
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    out = {}
    # kNN normals: the same sheet, shuffled and Morton-sorted
    m = args.follow_points
    sheet = sheet_cloud(torch, m, 42)
    cloud = pa.ExternalColumnsBuffer([sheet], layout, m)
    normals = torch.empty(m * 3, dtype=torch.float64, device="cuda")
    curvature = torch.empty(m, dtype=torch.float64, device="cuda")
    legs = {"shuffled": alg.shuffle(cloud, 1), "morton_sorted": alg.morton_sort(cloud)}
    out["compute_normals_k16"] = {"points": m}
    for name, buf in legs.items():
        def call():
            alg.compute_normals_device(buf, 16, normals.data_ptr(), curvature.data_ptr())
            hip.stream_synchronize()
        out["compute_normals_k16"][name] = quartiles(timed(torch, call, args.warmup, args.reps)[0])
    out["compute_normals_k16"]["shuffled_to_morton_sorted"] = round(out["compute_normals_k16"]["shuffled"]["median_ms"] /
                                                                    out["compute_normals_k16"]["morton_sorted"]["median_ms"], 4)
    del legs, sheet, cloud
    hip.release_scratch()
    # minimum-distance subsampling in index order: a scan-line ordered sheet as it is, and after shuffle
    m = args.index_points
    part = sheet_cloud(torch, m, 42)
    radius = math.sqrt(8.0 / (math.pi * m / 1.0e6))
    line = torch.floor(part[:, 1] / (4.0 * radius))
    lines = part[torch.argsort(line * 2048.0 + part[:, 0])].contiguous()
    scan = pa.ExternalColumnsBuffer([lines], layout, m)
    mask = torch.empty(m, dtype=torch.uint8, device="cuda")
    out["poisson_disk_index_order"] = {"points": m, "radius": radius}
    for name, buf in (("scan_line_input", scan), ("after_shuffle", alg.shuffle(scan, 1))):
        kept, rounds = C.c_uint64(), C.c_uint32()

        def call():
            hip.poisson_disk_mask(buf._h, radius, 1, 0, C.c_void_p(mask.data_ptr()), 0, C.byref(kept), C.byref(rounds))
        q = quartiles(timed(torch, call, 0, 1)[0])
        q.update({"rounds": int(rounds.value), "kept": int(kept.value)})
        out["poisson_disk_index_order"][name] = q
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--follow-points", type=int, default=10_000_000, help="points of the kNN normals leg")
    ap.add_argument("--index-points", type=int, default=1_000_000, help="points of the two index-order subsampling legs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="gather,orders,follow")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_reorder.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg, las
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    result = {"bench": "reorder", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.reorder_kernel_shape(hip)}
    legs = args.legs.split(",")
    if "gather" in legs:
        layouts = {"position3d": pa.PointLayout.from_attributes([A.POSITION_3D], api=hip),
                   "las0_typed": las.point_layout_from_las_point_format(las.Format(0), False, api=hip)}
        for lname, layout in layouts.items():
            for kname, kind in (("columnar", pa.HashMapBuffer), ("interleaved", pa.VectorBuffer)):
                result[f"gather_{lname}_{kname}"] = gather_legs(torch, pa, alg, hip, layout, kind, n, args)
                hip.release_scratch()
                torch.cuda.empty_cache()
    if "orders" in legs:
        result["sort_orders"] = order_legs(torch, pa, alg, hip, n, args)
        hip.release_scratch()
        torch.cuda.empty_cache()
    if "follow" in legs:
        result.update(follow_on_legs(torch, pa, alg, hip, args))
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
