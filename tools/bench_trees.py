#!/usr/bin/env python3
"""Tree tops and crowns on a synthetic stand: per point order one fresh child process under its own time limit, warm-up, timed repetitions
with device events, medians with their spread, one JSON line.

`--points` points at 10 per m^2 over rolling terrain under a stand of paraboloid crowns (one tree per 10 m x 10 m, jittered, 8 - 20 m tall,
crown radius a quarter of the height), each point's height above the terrain in a float64 DEVICE column -- what
pst_height_above_ground_device would have written -- in ONE columnar Position3D buffer, in two orders:
  random      as drawn
  scan_line   drawn in strips of about 2 m along y, one after the other, ascending x within a strip
Legs: a fixed window (r = 3 m) and the variable one (r = 1.5 + 0.1 h clamped to [1, 5]).  Measured per leg: pst_tree_tops_device (with the
index list), its phases (PST_TREES_TIMES=1, pst_trees_phase_times), how many candidates the near pass leaves to the far pass, and -- in one
more, untimed call of a second child started with PST_TREES_WORK=1 -- the candidates the far pass tests per top; then
pst_segment_trees_device on the variable leg's tops and its phases.  Yardsticks in the same process on the same buffers:
pst_height_above_ground_device with k = 1 (ground: the points below 0.5 m), pst_calculate_bounds; and, in a last child of its own because it
is the slowest line by far, pst_radius_outlier_mask at the fixed window's radius (one repetition).

    python tools/bench_trees.py [--points 100000000] [--reps 3] [--warmup 1] [--limit 900] [--out profiles/trees_1e8.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WINDOWS = {"fixed": (3.0, 0.0, 3.0, 3.0), "variable": (1.5, 0.1, 1.0, 5.0)}  # radii
MIN_HEIGHT = 2.0
PITCH = 10.0
DENSITY = 10.0


def say(text):
    print(text, file=sys.stderr, flush=True)


def _hash01(torch, i, j, salt):
    """a number in [0, 1) per lattice cell: the trees are a function of the cell, so a point finds its nine candidate trees without a table"""
    v = (i * 73856093) ^ (j * 19349663) ^ (salt * 83492791)
    v = (v * 2654435761) & 0xFFFFFFFF
    v = ((v ^ (v >> 15)) * 2246822519) & 0xFFFFFFFF
    v = v ^ (v >> 13)
    return v.to(torch.float64) / 4294967296.0


def stand_cloud(torch, n, seed, order):
    """(positions [n, 3], heights above the terrain [n], trees planted)"""
    side = math.sqrt(n / DENSITY)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if order == "random":
        xy = torch.rand(n, 2, device="cuda", dtype=torch.float64, generator=g) * side
    elif order == "scan_line":  # strips of about 2 m along y, drawn strip by strip: ascending x within a strip, y anywhere in it
        strips = max(1, int(side // 2.0))
        per, height = n // strips, side / strips
        xs = torch.sort(torch.rand(strips, per, device="cuda", dtype=torch.float64, generator=g) * side, dim=1).values
        ys = (torch.arange(strips, device="cuda", dtype=torch.float64)[:, None] + torch.rand(strips, per, device="cuda", dtype=torch.float64, generator=g)) * height
        rest = n - strips * per  # (one more, shorter line at the top)
        xr = torch.sort(torch.rand(rest, device="cuda", dtype=torch.float64, generator=g) * side).values
        yr = side - torch.rand(rest, device="cuda", dtype=torch.float64, generator=g) * height
        xy = torch.stack([torch.cat([xs.reshape(-1), xr]), torch.cat([ys.reshape(-1), yr])], dim=1).contiguous()
        del xs, ys, xr, yr
    else:
        sys.exit(f"unknown order {order!r}")
    h = torch.rand(n, device="cuda", dtype=torch.float64, generator=g) * 0.3
    for c0 in range(0, n, 10_000_000):
        p = xy[c0:c0 + 10_000_000]
        ci, cj = torch.floor(p[:, 0] / PITCH).to(torch.int64), torch.floor(p[:, 1] / PITCH).to(torch.int64)
        best = h[c0:c0 + 10_000_000]
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                i, j = ci + di, cj + dj
                tx = (i.to(torch.float64) + 0.5) * PITCH + 2.0 * _hash01(torch, i, j, 1) - 1.0
                ty = (j.to(torch.float64) + 0.5) * PITCH + 2.0 * _hash01(torch, i, j, 2) - 1.0
                H = 8.0 + 12.0 * _hash01(torch, i, j, 3)
                d2 = (p[:, 0] - tx) ** 2 + (p[:, 1] - ty) ** 2
                torch.maximum(best, H * (1.0 - d2 / (0.25 * H) ** 2), out=best)
    z = 0.02 * xy[:, 0] + 1.5 * torch.sin(xy[:, 0] / 15.0) * torch.cos(xy[:, 1] / 18.0) + h
    cells = int(side // PITCH) ** 2
    return torch.cat([xy, z[:, None]], dim=1).contiguous(), h, cells


def child(args):
    """One order of the cloud; prints its JSON object on the last line of stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_trees.py measures on the GPU; there is none here")
    import pasture_amd as pa
    from pasture_amd import algorithms as alg
    from pasture_amd.layout import attributes as A
    from bench_clusters import quartiles, timed

    hip = pa.product_api()
    n = args.points
    order, _, part = args.child.partition(":")
    layout = pa.PointLayout.from_attributes([A.POSITION_3D], api=hip)
    pos, h, planted = stand_cloud(torch, n, 42, order)
    buf = pa.ExternalColumnsBuffer([pos], layout, n)
    side = math.sqrt(n / DENSITY)
    lo, hi = pos[:, :2].min().item(), pos[:, :2].max().item()
    if not (0.0 <= lo and hi <= side and bool(torch.isfinite(pos).all()) and bool(torch.isfinite(h).all())):
        sys.exit(f"the cloud is not what it should be: x, y in [{lo}, {hi}], side {side}")
    out = {"trees_planted_about": planted, "points_at_or_above_min_height": int((h >= MIN_HEIGHT).sum())}
    if part == "outliers":
        mask, kept = torch.empty(n, dtype=torch.uint8, device="cuda"), C.c_uint64()
        r = WINDOWS["fixed"][0]
        out["radius_outlier_mask"] = {"radius": r, **quartiles(timed(torch, lambda: hip.radius_outlier_mask(buf._h, r, 8, C.c_void_p(mask.data_ptr()), 0, C.byref(kept)), 0, 1)[0])}
        print(json.dumps(out))
        return
    counting = part == "work"
    reps = 0 if counting else args.reps
    top = torch.empty(n, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n // 8, dtype=torch.int32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    out["legs"] = {}
    for name, window in WINDOWS.items():
        info = {}

        def call():
            info.update(alg.tree_tops_device(buf, window, MIN_HEIGHT, top.data_ptr(), h.data_ptr(), 0, 0.0, idx.data_ptr(), n // 8))
        if counting:
            call()
            w = alg.trees_work(hip)
            row = {"work": w, "far_tested_per_top": round(w["far_tested"] / max(1, info["n_tops"]), 2), "far_tested_per_survivor": round(w["far_tested"] / max(1, w["survivors"]), 2)}
        else:
            call()  # (untimed: the library must see the cloud torch made before anything is measured on it)
            w = alg.trees_work(hip)
            if w["candidates"] != out["points_at_or_above_min_height"]:
                sys.exit(f"{w['candidates']} candidates, but {out['points_at_or_above_min_height']} points at or above the floor")
            t, phases = timed(torch, call, args.warmup, reps, after=lambda: alg.trees_phase_times(hip))
            p = np.median(np.asarray(phases), axis=0)
            row = {"call": quartiles(t), "phases_ms": {"candidate_index": round(float(p[0]), 4), "filter": round(float(p[1]), 4), "numbering": round(float(p[2]), 4)},
                   "candidates": w["candidates"], "survivors_of_the_near_pass": w["survivors"], "n_tops": info["n_tops"], "cell_edge": info["cell_edge"], "dim": list(info["dim"])}
        out["legs"][name] = row
        say(f"  {order} {name}: {row}")
    if not counting:
        # the crowns on the variable leg's tops (`top` holds them)
        seg = {}

        def crowns():
            seg.update(alg.segment_trees_device(buf, top.data_ptr(), ids.data_ptr(), 0.6, 0.3, MIN_HEIGHT, h.data_ptr()))
        t, phases = timed(torch, crowns, args.warmup, reps, after=lambda: alg.trees_phase_times(hip))
        p = np.median(np.asarray(phases), axis=0)
        out["segment_trees"] = {"call": quartiles(t), "phases_ms": {"numbering": round(float(p[2]), 4), "top_index_and_crown_search": round(float(p[3]), 4)}, **seg}
        say(f"  {order} crowns: {out['segment_trees']}")
        # the yardsticks
        ground = (h < 0.5).to(torch.uint8)
        hag = torch.empty(n, dtype=torch.float64, device="cuda")
        t_hag = quartiles(timed(torch, lambda: alg.height_above_ground_device(buf, ground.data_ptr(), 1, hag_ptr=hag.data_ptr()), args.warmup, reps)[0])
        out["height_above_ground_k1"] = t_hag
        out["calculate_bounds"] = quartiles(timed(torch, lambda: alg.calculate_bounds(buf), args.warmup, reps)[0])
        for row in out["legs"].values():
            row["filter_to_height_above_ground"] = round(row["phases_ms"]["filter"] / t_hag["median_ms"], 3)
            row["call_to_height_above_ground"] = round(row["call"]["median_ms"] / t_hag["median_ms"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--orders", default="random,scan_line")
    ap.add_argument("--limit", type=int, default=900, help="seconds one child process may take; after a child that fails or runs out of time no other is started")
    ap.add_argument("--no-outliers", action="store_true", help="leave the radius-outlier yardstick out")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    result = {"bench": "trees", "points": args.points, "points_per_m2": DENSITY, "seed": 42, "windows_radii": WINDOWS, "min_height": MIN_HEIGHT}
    base = [sys.executable, os.path.abspath(__file__), "--points", str(args.points), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    steps = [(name, part) for name in args.orders.split(",") for part in ("timed", "work")]
    if not args.no_outliers:
        steps.append((args.orders.split(",")[0], "outliers"))
    ok = True
    for name, part in steps:
        result.setdefault(name, {})
        if not ok:
            result[name][part] = {"skipped": "an earlier step failed or ran out of time"}
            continue
        say(f"{name} ({part})")
        extra = {"timed": {"PST_TREES_TIMES": "1"}, "work": {"PST_TREES_WORK": "1"}, "outliers": {}}[part]
        try:
            r = subprocess.run(base + ["--child", f"{name}:{part}"], env=dict(os.environ, **extra), stdout=subprocess.PIPE, text=True, timeout=args.limit)
            ok = r.returncode == 0
            result[name][part] = json.loads(r.stdout.strip().splitlines()[-1]) if ok else {"failed": r.returncode}
        except subprocess.TimeoutExpired:
            ok = False
            result[name][part] = {"failed": f"no result within {args.limit} s"}
    try:
        import pasture_amd as pa
        result["kernel_shape"] = pa.trees_kernel_shape()
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
