#!/usr/bin/env python3
"""Ground classification (progressive morphological filter) on synthetic terrain: one fresh process, warm-up, timed repetitions with device
events, medians, one JSON line.

One cloud in two arrival orders, each in ONE columnar Position3D buffer: rolling terrain with 2 cm of noise and 2 % of the points lifted off
it, over a square sized so that a cell of the raster holds about `--per-cell` points.
  uniform    the points in random order: the filtered atomics of the raster and the reads of the classification scatter over the whole raster
  scanline   the same points sorted into scan lines (strips half a cell wide along x, x ascending inside a strip): neighbours in memory are
             neighbours on the ground, as a sensor delivers them
Reported: the whole pst_pmf_ground_mask call (mask to device memory), its three phases from stream events inside the call (PST_PMF_TIMES=1,
pst_pmf_phase_times), and pst_calculate_bounds on the same buffer in the same process -- the call reads the positions twice (three times
with its own bounds pass), so two to three bounds passes plus the raster traffic are its floor.

    python tools/bench_ground.py [--points 100000000] [--reps 5] [--warmup 1] [--out profiles/ground_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

os.environ["PST_PMF_TIMES"] = "1"  # read once, at the library's first ground call
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


def terrain_cloud(torch, n, side, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    xy = torch.rand(n, 2, device="cuda", dtype=torch.float64, generator=g) * side
    z = 10.0 * torch.sin(xy[:, 0] / 50.0) * torch.cos(xy[:, 1] / 80.0) + 50.0 + 0.02 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g)
    lifted = torch.rand(n, device="cuda", dtype=torch.float64, generator=g) < 0.02
    z = torch.where(lifted, z + 1.0 + 9.0 * torch.rand(n, device="cuda", dtype=torch.float64, generator=g), z)
    return torch.cat([xy, z[:, None]], dim=1).contiguous()


def measure(torch, alg, hip, buf, n, params, args):
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    count = C.c_uint64()

    def ground():
        hip.pmf_ground_mask(buf._h, *params.c_args(), C.c_void_p(mask.data_ptr()), 0, None, 0, C.byref(count))

    t_call, phases = timed(torch, ground, args.warmup, args.reps, after=lambda: alg.pmf_phase_times(hip))
    t_call = quartiles(t_call)
    phases = np.median(np.asarray(phases), axis=0)
    t_bounds = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    grid = alg.pmf_grid(buf, params.cell_size)
    return {"ground_points": int(count.value), "raster": {"cols": grid["cols"], "rows": grid["rows"], "points_per_cell": round(n / (grid["cols"] * grid["rows"]), 3)},
            "call": t_call, "points_per_second": round(n / (t_call["median_ms"] * 1e-3), 1),
            "phases_ms": {"bounds_and_raster": round(float(phases[0]), 4), "morphology": round(float(phases[1]), 4), "classification": round(float(phases[2]), 4)},
            "calculate_bounds": t_bounds, "ratio_to_calculate_bounds": round(t_call["median_ms"] / t_bounds["median_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--per-cell", type=float, default=10.0, help="points a cell of the raster should hold on average")
    ap.add_argument("--orders", default="uniform,scanline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ground.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A

    hip = pa.product_api()
    n = args.points
    params = pa.PmfParameters()  # 1 m cells, windows of 3 .. 33 cells
    side = math.sqrt(n / args.per_cell) * params.cell_size
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    half_widths, thresholds = alg.pmf_schedule(params, hip)
    result = {"bench": "ground", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.pmf_kernel_shape(hip),
              "parameters": {"cell_size": params.cell_size, "half_widths": half_widths.tolist(), "thresholds": thresholds.tolist()}, "side": round(side, 3)}
    cloud = terrain_cloud(torch, n, side, 42)
    for name in args.orders.split(","):
        if name == "scanline":
            key = torch.floor(cloud[:, 1] / (0.5 * params.cell_size)) * (2.0 * side) + cloud[:, 0]
            cloud = cloud[torch.argsort(key)].contiguous()
            del key
        elif name != "uniform":
            sys.exit(f"unknown order {name!r}")
        buf = pa.ExternalColumnsBuffer([cloud], layout, n)
        result[name] = measure(torch, alg, hip, buf, n, params, args)
        del buf
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
