#!/usr/bin/env python3
"""Height above ground (pst_height_above_ground_device) on synthetic terrain: warm-up, timed repetitions with device events, medians, and the
yardsticks on the same buffers in the same process; one JSON object, merged into --out leg by leg so that every leg can run in a process
and under a time limit of its own.

Legs:
  uniform / scanline   the terrain of tools/bench_ground.py (10 points per 1 m cell, 2 % of the points lifted off the ground) in random and in
                       scan-line order, the ground mask from pst_pmf_ground_mask; the buffer is its own ground.  k = 1 and k = 10, unbounded
                       and within three cell edges of the grid the call chose; the three phases from stream events inside the call
                       (PST_HAG_TIMES=1, pst_hag_phase_times).  Yardsticks: pst_calculate_bounds, pst_pmf_ground_mask, and
                       pst_nearest_neighbours_device of the non-ground points against an index over the ground points (the 3-D
                       one-neighbour search: fewer queries, an index built once outside the timing).
  boxes                the scene of examples/classify_ground.py with dense terrain: no ground under the boxes, so the roof centres are tens of
                       cells from any ground point.  Reported with the call's time: the rings a roof-centre query walks, replayed on the
                       host from the stop rule (smallest r >= 1 with d2 of the k-th nearest ground point <= (r * edge * (1 - 2^-20))^2).

    python tools/bench_hag.py [--points 100000000] [--legs uniform,scanline,boxes] [--reps 5] [--warmup 1] [--out profiles/hag_1e8.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import math
import os
import sys

import numpy as np

os.environ["PST_HAG_TIMES"] = "1"  # read once, at the library's first call
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ground import quartiles, terrain_cloud, timed  # noqa: E402


def hag_configs(torch, alg, hip, buf, mask, n, args):
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    first = alg.height_above_ground_device(buf, mask.data_ptr(), 10, hag_ptr=out.data_ptr())  # (also the warm-up of the process)
    result = {"n_ground": first["n_ground"]}
    for k in (1, 10):
        grid = alg.height_above_ground_device(buf, mask.data_ptr(), k, hag_ptr=out.data_ptr())
        for name, md in (("unbounded", float("inf")), ("within_3_edges", 3.0 * grid["cell_edge"])):
            info = {}

            def call():
                info.update(alg.height_above_ground_device(buf, mask.data_ptr(), k, md, hag_ptr=out.data_ptr()))
            t, phases = timed(torch, call, args.warmup, args.reps, after=lambda: alg.hag_phase_times(hip))
            t = quartiles(t)
            phases = np.median(np.asarray(phases), axis=0)
            result[f"k{k}_{name}"] = {"call": t, "points_per_second": round(n / (t["median_ms"] * 1e-3), 1), "max_distance": md if math.isfinite(md) else "inf", "n_unresolved": info["n_unresolved"],
                                      "grid": {"cell_edge": info["cell_edge"], "dim": list(info["dim"])},
                                      "phases_ms": {"ground_index": round(float(phases[0]), 4), "query_sort": round(float(phases[1]), 4), "search": round(float(phases[2]), 4)}}
    return result


def terrain_leg(torch, pa, alg, hip, cloud, n, params, args):
    from pasture_amd.layout import attributes as A
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    buf = pa.ExternalColumnsBuffer([cloud], layout, n)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    count = C.c_uint64()

    def ground():
        hip.pmf_ground_mask(buf._h, *params.c_args(), C.c_void_p(mask.data_ptr()), 0, None, 0, C.byref(count))
    t_pmf = quartiles(timed(torch, ground, args.warmup, args.reps)[0])
    t_bounds = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, args.reps)[0])
    result = hag_configs(torch, alg, hip, buf, mask, n, args)
    # the 3-D one-neighbour search the library already has: the non-ground points against an index over the ground points
    is_ground = mask.bool()
    ground_pts, other_pts = cloud[is_ground].contiguous(), cloud[~is_ground].contiguous()
    gbuf = pa.ExternalColumnsBuffer([ground_pts], layout, len(ground_pts))
    obuf = pa.ExternalColumnsBuffer([other_pts], layout, len(other_pts))
    index = alg.NearestNeighbourIndex(gbuf)
    dist = torch.empty(max(len(other_pts), 1), dtype=torch.float64, device="cuda")
    t_nn = quartiles(timed(torch, lambda: alg.nearest_neighbours_device(obuf, index, dist_ptr=dist.data_ptr()), args.warmup, args.reps)[0])
    index.destroy()
    result["yardsticks"] = {"calculate_bounds": t_bounds, "pmf_ground_mask": t_pmf,
                            "nearest_neighbours_3d": dict(t_nn, queries=len(other_pts), targets=len(ground_pts))}
    for key, cfg in result.items():
        if key.startswith("k"):
            cfg["ratios"] = {"to_calculate_bounds": round(cfg["call"]["median_ms"] / t_bounds["median_ms"], 3),
                             "to_pmf_ground_mask": round(cfg["call"]["median_ms"] / t_pmf["median_ms"], 3),
                             "to_nearest_neighbours_3d": round(cfg["call"]["median_ms"] / t_nn["median_ms"], 3)}
    return result


def boxes_leg(torch, pa, alg, hip, n_terrain, args):
    from pasture_amd.layout import attributes as A
    spec = importlib.util.spec_from_file_location("classify_ground_scene", os.path.join(ROOT, "examples", "classify_ground.py"))
    scene = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene)
    pts, owner = scene.scene(n_terrain)
    roofs = np.array([[cx, cy, scene.height(cx, cy) + scene.CLEAR + h] for cx, cy, _, _, h in scene.OBJECTS[:3]])  # the roof centres, as queries
    pts, owner = np.concatenate([pts, roofs]), np.concatenate([owner, [0, 1, 2]])
    n = len(pts)
    cloud = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    mask = torch.from_numpy((owner < 0).astype(np.uint8)).cuda()  # the terrain itself is the ground set here: the leg measures the walk, not the filter
    buf = pa.ExternalColumnsBuffer([cloud], pa.PointLayout.from_attributes([A.POSITION_3D], api=hip), n)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    result = {"points": n, "terrain_points": int((owner < 0).sum())}
    ground_xy = pts[owner < 0][:, :2]
    for k in (1, 10):
        info = {}

        def call():
            info.update(alg.height_above_ground_device(buf, mask.data_ptr(), k, hag_ptr=out.data_ptr()))
        t, phases = timed(torch, call, args.warmup, args.reps, after=lambda: alg.hag_phase_times(hip))
        phases = np.median(np.asarray(phases), axis=0)
        edge_stop = info["cell_edge"] * (1.0 - 2.0 ** -20)
        rings = []
        for q in roofs:
            d2 = np.sort(((ground_xy - q[:2]) ** 2).sum(axis=1))[k - 1]
            rings.append(max(1, int(math.ceil(math.sqrt(d2) / edge_stop))))
        result[f"k{k}"] = {"call": quartiles(t), "grid": {"cell_edge": info["cell_edge"], "dim": list(info["dim"])}, "n_unresolved": info["n_unresolved"],
                           "phases_ms": {"ground_index": round(float(phases[0]), 4), "query_sort": round(float(phases[1]), 4), "search": round(float(phases[2]), 4)},
                           "roof_centre_rings_walked": rings, "roof_centre_hag": [round(float(v), 3) for v in out[-3:].cpu().numpy()]}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--box-terrain-points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--per-cell", type=float, default=10.0, help="points a 1 m cell of the ground filter's raster should hold on average")
    ap.add_argument("--legs", default="uniform,scanline,boxes")
    ap.add_argument("--out", default=None, help="merged into: legs already there are kept")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_hag.py measures on the GPU; there is none here")
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
    result.update({"bench": "hag", "points": n, "seed": 42, "device": torch.cuda.get_device_name(0), "kernel_shape": alg.hag_kernel_shape(hip), "side": round(side, 3)})
    legs = args.legs.split(",")
    cloud = terrain_cloud(torch, n, side, 42) if ("uniform" in legs or "scanline" in legs) else None
    for name in legs:
        if name == "boxes":
            result[name] = boxes_leg(torch, pa, alg, hip, args.box_terrain_points, args)
            continue
        if name == "scanline":
            key = torch.floor(cloud[:, 1] / (0.5 * params.cell_size)) * (2.0 * side) + cloud[:, 0]
            pts = cloud[torch.argsort(key)].contiguous()
            del key
        elif name == "uniform":
            pts = cloud
        else:
            sys.exit(f"unknown leg {name!r}")
        result[name] = terrain_leg(torch, pa, alg, hip, pts, n, params, args)
        del pts
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
