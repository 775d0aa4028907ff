"""Forest metrics on the device: the stand of tree_inventory.py -> progressive morphological filter -> height above ground -> per 10 m cell
the median and the 95th percentile of the heights and the canopy cover (the share of returns above 2 m) -> tree tops and crowns -> per tree
the 95th height percentile next to the largest height and the height the tree was planted with.

What a lidR user writes as pixel_metrics(~list(zq50, zq95, pzabove2), 10) and crown_metrics(~quantile(Z, 0.95)), and a PDAL user as
filters.stats with percentiles per raster cell.  Only the two small tables leave the device.  Usage:

    python examples/forest_metrics.py [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from tree_inventory import MIN_HEIGHT, STAND, WINDOW, scene

CELL = 10.0
COVER_ABOVE = 2.0


def metrics(n_points=60_000, seed=3, verbose=False):
    say = print if verbose else (lambda *a: None)
    pts, trunks, planted = scene(n_points, seed)
    n = len(pts)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)

    # 1. the ground, 2. every point's height above it: a device column that never leaves the device
    pa.classify_ground(cloud, pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2))
    ground, hag = _DeviceArray(cloud.api, T.U8, n), _DeviceArray(cloud.api, T.F64, n)
    pa.classification_mask(cloud, 2, ground.ptr)
    pa.height_above_ground_device(cloud, ground.ptr, k=3, hag_ptr=hag.ptr)

    # 3. per 10 m cell: p50 and p95 of the heights, and the cover above 2 m
    r = pa.rasterize_quantiles(cloud, CELL, probs=(0.5, 0.95), above=(COVER_ABOVE,), values=hag.ptr)
    count, (p50, p95), above = r.planes["count"], r.planes["quantiles"], r.planes["above"][0]
    with np.errstate(invalid="ignore"):
        cover = above / count
    in_stand = np.zeros_like(count, dtype=bool)
    in_stand[:, :int(STAND // CELL)] = count[:, :int(STAND // CELL)] > 0  # (the strip beside the stand holds two boxes and bare ground)
    say(f"{n} points on a grid of {r.cols} x {r.rows} cells of {CELL} m; in the stand: median p50 {np.median(p50[in_stand]):.2f} m, median p95 {np.median(p95[in_stand]):.2f} m, "
        f"cover above {COVER_ABOVE} m {100.0 * above[in_stand].sum() / count[in_stand].sum():.1f} %")

    # 4. per tree: p95 of the heights of its crown next to the largest one and the planted height
    tops = pa.tree_tops(cloud, window=WINDOW, min_height=MIN_HEIGHT, heights=hag.ptr)
    labels = _DeviceArray(cloud.api, T.U32, n)
    seg = pa.segment_trees(cloud, tops, max_crown_factor=0.6, exclusion=0.3, min_height=MIN_HEIGHT, heights=hag.ptr, device_tree_id_ptr=labels.ptr)
    q = pa.segment_quantiles(cloud, labels.ptr, seg.n_trees, probs=(0.95,), above=(COVER_ABOVE,), values=hag.ptr)
    table = pa.segment_statistics(cloud, labels.ptr, seg.n_trees, ("count", "value_max"), values=hag.ptr)
    assert np.array_equal(q.count, table.count)
    # the tree a top stands for: the planted trunk nearest to it
    top_xy = pts[tops.indices.astype(np.int64), :2]
    d2 = ((top_xy[:, None, :] - trunks[None, :, :]) ** 2).sum(axis=2)
    nearest = d2.argmin(axis=1)
    rows = [(t, float(q.quantiles[0][t]), float(table.value_max[t]), float(planted[nearest[t]]), int(q.count[t])) for t in range(seg.n_trees)
            if d2[t, nearest[t]] < 1.0]  # (a top on the shed's roof stands for no tree)
    say(f"{seg.n_trees} crowns; the five tallest (p95 of the crown's heights, its largest height, the height planted, points):")
    for t, p, top, h, c in rows[:5]:
        say(f"  tree {t}: p95 {p:6.2f} m, max {top:6.2f} m, planted {h:6.2f} m, {c} points")
    return {"cols": r.cols, "rows": r.rows, "p50": p50, "p95": p95, "cover": cover, "in_stand": in_stand, "trees": rows, "planted": len(trunks)}


if __name__ == "__main__":
    metrics(int(sys.argv[1]) if len(sys.argv) > 1 else 60_000, verbose=True)
