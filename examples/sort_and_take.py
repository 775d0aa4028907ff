"""Index lists put to use on the device: sort a cloud by an attribute, take the points an index list names, reorder for locality and carry a
per-point result back.

A synthetic LAS-like cloud (a tilted ground plane with clutter above it, GpsTime in acquisition order but stored shuffled):
  1. sort_by_attribute(GpsTime)      PDAL's filters.sort: the points back in acquisition order;
  2. ransac_plane, plane_inliers     the ground plane and the u64 index list of its inliers;
  3. take(inliers)                   "the inliers as a buffer", every attribute, without a host round trip of the points;
  4. calculate_bounds                of the taken points;
  5. morton_sort + invert_order      the cloud in Z-order (neighbours in space become neighbours in memory), a per-point result computed on
                                     the sorted cloud -- here the kNN curvature -- carried back to the input order.
Usage:

    python examples/sort_and_take.py [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import attributes as A


def cloud(n, rng):
    """(positions, gps time, intensity, classification): 70 % ground on the plane z = 0.02 x - 0.01 y + 100 (2 cm noise), the rest up to 30 m above"""
    xy = rng.random((n, 2)) * 500.0
    ground = rng.random(n) < 0.7
    z = 0.02 * xy[:, 0] - 0.01 * xy[:, 1] + 100.0 + np.where(ground, rng.normal(0, 0.02, n), rng.random(n) * 30.0 + 1.0)
    gps = np.sort(rng.random(n) * 3600.0)            # acquisition order ...
    shuffled = rng.permutation(n)                    # ... lost on the way here
    pos = np.column_stack([xy, z])[shuffled]
    return pos, gps[shuffled], rng.integers(0, 4096, n).astype(np.uint16)[shuffled], np.where(ground, 2, 1).astype(np.uint8)[shuffled]


def main(n=200_000):
    rng = np.random.default_rng(3)
    pos, gps, intensity, classification = cloud(n, rng)
    layout = pa.PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY, A.CLASSIFICATION, A.GPS_TIME])
    buf = pa.HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    for attribute, values in ((A.POSITION_3D, pos), (A.INTENSITY, intensity), (A.CLASSIFICATION, classification), (A.GPS_TIME, gps)):
        buf.set_attribute_range(attribute, range(0, n), values)

    # 1. back into acquisition order
    by_time = pa.sort_by_attribute(buf, A.GPS_TIME)
    t = by_time.view_attribute(A.GPS_TIME)
    assert (np.diff(t) >= 0).all()
    print(f"{n} points sorted by GpsTime: {t[0]:.3f} s .. {t[-1]:.3f} s")

    # 2. + 3. the ground plane, its inliers as an index list, the inliers as a buffer
    plane, _ = pa.ransac_plane(by_time, 0.1, 200, seed=1)
    inliers = pa.plane_inliers(by_time, plane, 0.1)
    ground = by_time.take(inliers)
    share = float((ground.view_attribute(A.CLASSIFICATION) == 2).mean())
    print(f"plane {tuple(round(c, 4) for c in plane.coefficients())}: {len(inliers)} inliers taken, {100 * share:.1f} % of them classified ground")
    assert ground.len() == len(inliers) and np.array_equal(ground.view_attribute(A.GPS_TIME), t[inliers.astype(np.int64)])

    # 4. bounds of the taken points
    bounds = pa.calculate_bounds(ground)
    print(f"bounds of the inliers: {tuple(round(v, 2) for v in bounds.min())} .. {tuple(round(v, 2) for v in bounds.max())}")

    # 5. Z-order for locality; a result of the sorted cloud carried back to the input order
    sorted_buf, order = pa.morton_sort(by_time, return_order=True)
    _, curvature_sorted = pa.compute_normals(sorted_buf, 16)
    inverse = pa.invert_order(order)
    curvature = curvature_sorted[inverse]            # curvature[i] belongs to point i of by_time
    _, direct = pa.compute_normals(by_time, 16)
    print(f"curvature via the Morton-sorted cloud vs computed in place: max |difference| {float(np.nanmax(np.abs(curvature - direct))):.3e}")
    flat = curvature[inliers.astype(np.int64)]
    print(f"median curvature: inliers {float(np.nanmedian(flat)):.2e}, all points {float(np.nanmedian(curvature)):.2e}")
    return len(inliers), share


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
