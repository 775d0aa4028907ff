#!/usr/bin/env python3
"""Rasterisation (pst_rasterize, pst_grid_fill_device) on synthetic terrain: warm-up, timed repetitions with device events, medians with
their spread, and the yardsticks on the same buffer in the same process; one JSON object, merged into --out leg by leg so that every leg can
run in a process and under a time limit of its own.

Legs:
  uniform / scanline   the terrain of tools/bench_ground.py (10 points per 1 m cell) in random and in scan-line order, z as the value, planes
                       in device memory: MAX alone and COUNT | MIN | MAX (the atomic path), all five statistics (the sorted path) with the
                       three phases from stream events inside the call (PST_RASTER_TIMES=1, pst_raster_phase_times), and MAX alone on the
                       same grid GIVEN by the caller (no bounds pass).  Yardsticks: pst_calculate_bounds and pst_pmf_ground_mask with its
                       phases.
  fill                 pst_grid_fill_device at half-widths 1 and 8 on the MAX raster of the uniform cloud with 5 % of its cells emptied.
  onecell              --onecell-points points in ONE cell, all five statistics: whether one lane sums a whole cell.

    python tools/bench_raster.py [--points 100000000] [--legs uniform,scanline,fill,onecell] [--reps 5] [--warmup 1] [--out profiles/raster_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_RASTER_TIMES"] = "1"  # read once, at the library's first call
os.environ["PST_PMF_TIMES"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ground import quartiles, terrain_cloud, timed  # noqa: E402

CONFIGS = {"max": ("max",), "count_min_max": ("count", "min", "max"), "all_five": ("count", "min", "max", "mean", "variance")}


def raster_call(torch, alg, hip, buf, cell, stats, out, args, **kw):
    info = {}

    def call():
        info["r"] = alg.rasterize(buf, cell, stats, device_out_ptr=out.data_ptr(), **kw)
    t, phases = timed(torch, call, args.warmup, args.reps, after=lambda: alg.raster_phase_times(hip))
    phases = np.median(np.asarray(phases), axis=0)
    r = info["r"]
    return {"call": quartiles(t), "n_members": r.n_members, "cols": r.cols, "rows": r.rows,
            "phases_ms": {"bounds": round(float(phases[0]), 4), "keys_sort_directory": round(float(phases[1]), 4), "reduction_and_output": round(float(phases[2]), 4)}}


def terrain_leg(torch, pa, alg, hip, cloud, n, params, args):
    from pasture_amd.layout import attributes as A
    buf = pa.ExternalColumnsBuffer([cloud], pa.PointLayout.from_attributes([A.POSITION_3D], api=hip), n)
    grid = alg.pmf_grid(buf, params.cell_size)
    cols, rows = grid["cols"], grid["rows"]
    out = torch.empty((5, rows, cols), dtype=torch.float64, device="cuda")
    result = {"raster": {"cols": cols, "rows": rows, "points_per_cell": round(n / (cols * rows), 3)}}
    for name, stats in CONFIGS.items():
        result[name] = raster_call(torch, alg, hip, buf, params.cell_size, stats, out, args)
    result["max_given_grid"] = raster_call(torch, alg, hip, buf, params.cell_size, ("max",), out, args, origin=grid["origin"], dim=(cols, rows))
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    count = C.c_uint64()

    def ground():
        hip.pmf_ground_mask(buf._h, *params.c_args(), C.c_void_p(mask.data_ptr()), 0, None, 0, C.byref(count))
    t_pmf, phases = timed(torch, ground, args.warmup, args.reps, after=lambda: alg.pmf_phase_times(hip))
    phases = np.median(np.asarray(phases), axis=0)
    t_pmf, t_bounds = quartiles(t_pmf), quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    result["yardsticks"] = {"calculate_bounds": t_bounds, "pmf_ground_mask": dict(t_pmf, phases_ms={"bounds_and_raster": round(float(phases[0]), 4),
                                                                                                   "morphology": round(float(phases[1]), 4),
                                                                                                   "classification": round(float(phases[2]), 4)})}
    for name in list(CONFIGS) + ["max_given_grid"]:
        result[name]["points_per_second"] = round(n / (result[name]["call"]["median_ms"] * 1e-3), 1)
        result[name]["ratios"] = {"to_calculate_bounds": round(result[name]["call"]["median_ms"] / t_bounds["median_ms"], 3),
                                  "to_pmf_ground_mask": round(result[name]["call"]["median_ms"] / t_pmf["median_ms"], 3)}
    return result, out[0], cols, rows


def fill_leg(torch, alg, hip, raster, cols, rows, args):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    holed = raster.clone()
    holed[torch.rand((rows, cols), device="cuda", generator=g) < 0.05] = float("nan")
    filled = torch.empty_like(holed)
    result = {"cols": cols, "rows": rows, "empty_cells": int(torch.isnan(holed).sum().item())}
    for h in (1, 8):
        t = quartiles(timed(torch, lambda: alg.grid_fill(holed.data_ptr(), filled.data_ptr(), cols, rows, h, hip), args.warmup, args.reps)[0])
        result[f"h{h}"] = dict(t, cells_per_second=round(cols * rows / (t["median_ms"] * 1e-3), 1), left_empty=int(torch.isnan(filled).sum().item()))
    return result


def onecell_leg(torch, pa, alg, hip, n, args):
    from pasture_amd.layout import attributes as A
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    cloud = torch.rand(n, 3, device="cuda", dtype=torch.float64, generator=g)
    buf = pa.ExternalColumnsBuffer([cloud], pa.PointLayout.from_attributes([A.POSITION_3D], api=hip), n)
    out = torch.empty((5, 1, 1), dtype=torch.float64, device="cuda")
    result = raster_call(torch, alg, hip, buf, 2.0, CONFIGS["all_five"], out, args)
    mean, var = out[3, 0, 0].item(), out[4, 0, 0].item()
    result.update(points=n, mean=mean, variance=var, torch_mean=cloud[:, 2].mean().item(), torch_variance=cloud[:, 2].var(unbiased=False).item())
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--onecell-points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--per-cell", type=float, default=10.0, help="points a 1 m cell should hold on average")
    ap.add_argument("--legs", default="uniform,scanline,fill,onecell")
    ap.add_argument("--out", default=None, help="merged into: legs already there are kept")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_raster.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg

    hip = pa.product_api()
    n = args.points
    params = pa.PmfParameters()
    side = math.sqrt(n / args.per_cell) * params.cell_size
    result = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result.update({"bench": "raster", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.raster_kernel_shape(hip), "side": round(side, 3)})
    legs = args.legs.split(",")
    cloud = terrain_cloud(torch, n, side, 42) if any(leg in legs for leg in ("uniform", "scanline", "fill")) else None
    raster = None
    for name in legs:
        if name == "onecell":
            result[name] = onecell_leg(torch, pa, alg, hip, args.onecell_points, args)
        elif name == "fill":
            if raster is None:
                from pasture_amd.layout import attributes as A
                buf = pa.ExternalColumnsBuffer([cloud], pa.PointLayout.from_attributes([A.POSITION_3D], api=hip), n)
                grid = alg.pmf_grid(buf, params.cell_size)
                raster = (torch.empty((grid["rows"], grid["cols"]), dtype=torch.float64, device="cuda"), grid["cols"], grid["rows"])
                alg.rasterize(buf, params.cell_size, ("max",), device_out_ptr=raster[0].data_ptr())
            result[name] = fill_leg(torch, alg, hip, *raster, args)
        elif name in ("uniform", "scanline"):
            if name == "scanline":
                key = torch.floor(cloud[:, 1] / (0.5 * params.cell_size)) * (2.0 * side) + cloud[:, 0]
                pts = cloud[torch.argsort(key)].contiguous()
                del key
            else:
                pts = cloud
            result[name], plane, cols, rows = terrain_leg(torch, pa, alg, hip, pts, n, params, args)
            if name == "uniform":
                raster = (plane.clone(), cols, rows)  # MAX of z: what the fill leg fills
            del pts, plane
        else:
            sys.exit(f"unknown leg {name!r}")
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
