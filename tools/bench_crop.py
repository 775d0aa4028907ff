#!/usr/bin/env python3
"""Polygon crop on synthetic points: one fresh process, warm-up, timed repetitions with device events, medians, one JSON line.

Clouds of --points points over 1000 x 1000: a uniform box and the LiDAR-like sheet of bench.py's kNN leg, each as generated and after
morton_sort.  Sets: a 4-edge square over half the area, a 64-edge and a 4 096-edge star, and 10^4 rectangles ("footprints").  Each set runs
with the mask and with the ids, under both kernels where the flat one is allowed.  The crossover legs run both kernels on the uniform cloud
at stars of 4, 64, 512 and flat_max_edges edges.  Baselines on the same buffers: pst_plane_inlier_mask_device (the nearest existing one-pass
mask kernel), pst_calculate_bounds, and crop end to end against filter with an all-ones mask.

    python tools/bench_crop.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/crop_1e8.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clusters import quartiles, sheet_cloud, timed  # noqa: E402

EXTENT = 1000.0


def star(n_vertices, r_outer=450.0, r_inner=200.0, phase=0.1):
    a = phase + 2.0 * np.pi * np.arange(n_vertices) / n_vertices
    r = np.where(np.arange(n_vertices) % 2 == 0, r_outer, r_inner)
    return np.column_stack([EXTENT / 2 + r * np.cos(a), EXTENT / 2 + r * np.sin(a)])


def rectangle(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def polygon_sets():
    half = EXTENT / np.sqrt(2.0) / 2.0
    return {"square_4": [rectangle(EXTENT / 2 - half, EXTENT / 2 - half, EXTENT / 2 + half, EXTENT / 2 + half)],
            "star_64": [star(64)],
            "star_4096": [star(4096)],
            "footprints_10000": [rectangle(10.0 * i + 2.0, 10.0 * j + 3.0, 10.0 * i + 8.0, 10.0 * j + 7.0) for j in range(100) for i in range(100)]}


def query_legs(torch, alg, hip, buf, n, polygons, kernels, args):
    """the mask and the ids under each kernel; bytes: the 24-byte positions in, 1 or 4 bytes out"""
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    out = {}
    for kernel in kernels:
        ps = alg.PolygonSet(polygons, kernel=kernel, api=hip)
        info = ps.info
        count = C.c_uint64()
        hip.polygon_mask_device(ps._h, buf._h, 0, C.c_void_p(mask.data_ptr()), C.byref(count))

        def run_mask():
            hip.polygon_mask_device(ps._h, buf._h, 0, C.c_void_p(mask.data_ptr()), None)
            hip.stream_synchronize()

        def run_ids():
            hip.points_in_polygons_device(ps._h, buf._h, C.c_void_p(ids.data_ptr()))
            hip.stream_synchronize()
        leg = {"entries": info["entries"], "bands": info["bands"], "directory_entries": info["directory_entries"], "inside": int(count.value)}
        for name, call, out_bytes in (("mask", run_mask, 1), ("ids", run_ids, 4)):
            q = quartiles(timed(torch, call, args.warmup, args.reps)[0])
            q["GB_per_s_wanted_bytes"] = round((24 + out_bytes) * n / q["median_ms"] / 1e6, 1)
            q["ns_per_point"] = round(q["median_ms"] * 1e6 / n, 4)
            leg[name] = q
        out[kernel] = leg
        ps.destroy()
    if "flat" in out and "banded" in out:
        assert out["flat"]["inside"] == out["banded"]["inside"]
        out["flat_to_banded_mask"] = round(out["flat"]["mask"]["median_ms"] / out["banded"]["mask"]["median_ms"], 4)
    return out


def baseline_legs(torch, pa, alg, hip, buf, n, sets, args, end_to_end):
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, -50.0)

    def plane_mask():
        hip.plane_inlier_mask_device(buf._h, plane, 5.0, C.c_void_p(mask.data_ptr()))
        hip.stream_synchronize()
    out = {"plane_inlier_mask": quartiles(timed(torch, plane_mask, args.warmup, args.reps)[0]),
           "calculate_bounds": quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])}
    if end_to_end:
        ps = alg.PolygonSet(sets["square_4"], api=hip)
        ones = torch.ones(n, dtype=torch.uint8, device="cuda")
        out["crop_square_end_to_end"] = quartiles(timed(torch, lambda: alg.crop(buf, ps, out_buffer_type=pa.HashMapBuffer), args.warmup, args.reps)[0])
        out["filter_all_ones"] = quartiles(timed(torch, lambda: buf.filter(pa.HashMapBuffer, (ones.data_ptr(), "device")), args.warmup, args.reps)[0])
        ps.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_crop.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    shape = alg.crop_kernel_shape(hip)
    result = {"bench": "crop", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": shape}
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    sets = polygon_sets()
    g = torch.Generator(device="cuda")
    g.manual_seed(42)
    sources = {"uniform_box": lambda: torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g) * torch.tensor([EXTENT, EXTENT, 100.0], device="cuda", dtype=torch.float64),
               "sheet": lambda: sheet_cloud(torch, n, 42)}
    for cname, make in sources.items():
        pts = make().contiguous()
        as_generated = pa.ExternalColumnsBuffer([pts], layout, n)
        for order, buf in (("as_generated", as_generated), ("morton_sorted", None)):
            if buf is None:
                buf = alg.morton_sort(as_generated, 2)
            legs = {}
            for sname, polygons in sets.items():
                n_entries = sum(2 if len(p) == 4 else len(p) for p in polygons)  # (a rectangle has two horizontal edges, the stars none)
                kernels = (["flat"] if n_entries <= shape["flat_max_edges"] else []) + ["banded"]
                legs[sname] = query_legs(torch, alg, hip, buf, n, polygons, kernels, args)
            legs["baselines"] = baseline_legs(torch, pa, alg, hip, buf, n, sets, args, end_to_end=(cname == "uniform_box" and order == "as_generated"))
            legs["square_mask_to_plane_mask"] = round(min(legs["square_4"][k]["mask"]["median_ms"] for k in ("flat", "banded")) /
                                                      legs["baselines"]["plane_inlier_mask"]["median_ms"], 4)
            if cname == "uniform_box" and order == "as_generated":  # both kernels at 4, 64, 512 and flat_max_edges edges: where does the flat one stop winning?
                cross = {}
                for edges in (4, 64, 512, shape["flat_max_edges"]):
                    cross[f"star_{edges}"] = query_legs(torch, alg, hip, buf, n, [star(edges)], ["flat", "banded"], args)
                legs["crossover"] = cross
            result[f"{cname}_{order}"] = legs
            del buf
            hip.release_scratch()
        del as_generated, pts
        torch.cuda.empty_cache()
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
