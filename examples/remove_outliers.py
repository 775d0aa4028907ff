"""Cleaning a cloud on the device: stray returns -> statistical / radius outlier masks -> compaction -> normals of what is left.

What a PCL or PDAL user writes with StatisticalOutlierRemoval / RadiusOutlierRemoval between "read" and "normals": the neighbour search, the
distances, the statistics, the mask and the compaction all stay in device memory.  Usage:

    python examples/remove_outliers.py [points] [strays]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition, PointLayout, attributes as A


def scene(n, strays, seed=7):
    """A gently rolling terrain with 5 cm of noise, and `strays` returns from nowhere (birds, multipath) scattered far around it."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 500.0
    z = 20.0 * np.sin(xy[:, 0] / 40.0) * np.cos(xy[:, 1] / 55.0) + rng.normal(0.0, 0.05, n)
    ground = np.column_stack([xy, z])
    far = ground.mean(axis=0) + (rng.random((strays, 3)) - 0.5) * 50000.0
    pts = np.concatenate([ground, far])
    order = rng.permutation(len(pts))
    return pts[order], order >= n


def main(n=200_000, strays=200):
    pts, is_stray = scene(n, strays)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    before = pa.calculate_bounds(cloud)
    print(f"{len(pts)} points, {strays} of them strays; bounds {before.min()} .. {before.max()}")

    # the neighbour lists on their own, with distances
    idx, dist = pa.knn_search(cloud.slice(range(0, 1000)), 4)
    print("point 0 of the first 1000: neighbours", idx[0], "at", dist[0])

    # statistical: mean distance to the 8 nearest neighbours against the mean + 1 stddev of all such means
    clean, st = pa.remove_statistical_outliers(cloud, 8, 1.0)
    b = pa.calculate_bounds(clean)
    print(f"statistical: mean {st.mean:.4f} stddev {st.stddev:.4f} threshold {st.threshold:.4f}; kept {st.kept} of {st.count}; bounds {b.min()} .. {b.max()}")

    # radius: at least 8 other points within 10 m; the mask alone first (a numpy array), then the compaction
    mask, kept = pa.radius_outlier_mask(cloud, 10.0, 8)
    print(f"radius: kept {kept}; strays among them: {int(mask[is_stray].sum())}; ground points lost: {int((1 - mask[~is_stray]).sum())}")
    clean2, kept2 = pa.remove_radius_outliers(cloud, 10.0, 8)
    assert kept2 == kept == clean2.len()

    # ... and on to the normals of the cleaned cloud
    normals = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.NORMAL, PointAttributeDefinition("Curvature", T.F64)]))
    normals.resize(clean.len())
    pa.compute_normals_into(clean, 16, normals)
    print("first normal of the cleaned cloud:", normals.view_attribute(A.NORMAL)[0])
    return st, kept, clean.len(), int(mask[is_stray].sum())


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
