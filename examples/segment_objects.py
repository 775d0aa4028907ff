"""From a cloud to objects on the device: terrain with a few boxes and poles on it -> RANSAC ground plane -> drop the ground -> Euclidean
clusters -> the bounds of the three largest objects.

What a PCL user writes with SACSegmentation + ExtractIndices + EuclideanClusterExtraction: the plane fit, both masks, both compactions, the
fixed-radius traversal and the connected components all stay in device memory.  Usage:

    python examples/segment_objects.py [ground points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

# (centre x, centre y, size x, size y, height): three boxes of decreasing size and two thin poles
OBJECTS = [(30.0, 30.0, 12.0, 8.0, 6.0), (70.0, 25.0, 6.0, 6.0, 4.0), (50.0, 75.0, 4.0, 3.0, 2.5), (15.0, 80.0, 0.3, 0.3, 8.0), (85.0, 85.0, 0.3, 0.3, 6.0)]
SPACING = 0.25  # point spacing on the objects' surfaces


def scene(n_ground, seed=11):
    """A 100 m x 100 m tilted plane with 2 cm of noise, and the objects' tops and walls sampled every SPACING, standing 1 m clear of the ground
    fit's threshold.  Returns (points, object number per point or -1 for the ground), shuffled."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n_ground, 2)) * 100.0
    ground = np.column_stack([xy, 0.02 * xy[:, 0] - 0.01 * xy[:, 1] + rng.normal(0.0, 0.02, n_ground)])
    parts, owner = [ground], [np.full(n_ground, -1)]
    for k, (cx, cy, sx, sy, h) in enumerate(OBJECTS):
        base = 0.02 * cx - 0.01 * cy + 1.0
        xs = np.arange(cx - sx / 2, cx + sx / 2 + 1e-9, SPACING)
        ys = np.arange(cy - sy / 2, cy + sy / 2 + 1e-9, SPACING)
        zs = np.arange(base, base + h + 1e-9, SPACING)
        top = np.array([(x, y, zs[-1]) for x in xs for y in ys])
        walls = np.array([(x, y, z) for z in zs[:-1] for x in xs for y in (ys[0], ys[-1])] + [(x, y, z) for z in zs[:-1] for y in ys[1:-1] for x in (xs[0], xs[-1])])
        obj = np.concatenate([top, walls])
        parts.append(obj)
        owner.append(np.full(len(obj), k))
    pts, owner = np.concatenate(parts), np.concatenate(owner)
    order = rng.permutation(len(pts))
    return pts[order], owner[order]


def main(n_ground=200_000):
    pts, owner = scene(n_ground)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    print(f"{len(pts)} points: {n_ground} on the ground, {int((owner >= 0).sum())} on {len(OBJECTS)} objects")

    # the ground: the plane most points lie within 15 cm of
    plane, inliers = pa.ransac_plane(cloud, 0.15, 256, seed=3)
    print(f"ground plane {tuple(round(c, 4) for c in plane.coefficients())}: {plane.ranking} inliers")

    # drop it: inlier mask on the device, inverted through its indices on the host side of the example only for the printout
    mask = _DeviceArray(cloud.api, T.U8, cloud.len())
    pa.plane_inlier_mask(cloud, plane, 0.15, mask.ptr)
    keep = 1 - mask.to_numpy()
    rest = cloud.filter(pa.HashMapBuffer, keep)
    print(f"{rest.len()} points left above the ground")

    # clusters: two points belong together when they are closer than two spacings; at least 50 points make an object
    tolerance = 2.0 * SPACING
    labels, sizes = pa.euclidean_clusters(rest, tolerance, min_size=50)
    print(f"{len(sizes)} objects of {sizes.tolist()} points; {int((labels == pa.NO_CLUSTER).sum())} points in none")

    # the three largest, each extracted on the device (labels and mask never leave it)
    rest_owner = owner[keep.astype(bool)]
    found = []
    for c in range(min(3, len(sizes))):
        obj, _ = pa.extract_clusters(rest, tolerance, min_size=50, first_cluster=c, cluster_count=1)
        b = pa.calculate_bounds(obj)
        found.append(int(np.bincount(rest_owner[labels == c] + 1).argmax()) - 1)
        print(f"object {c}: {obj.len()} points, bounds {tuple(round(v, 2) for v in b.min())} .. {tuple(round(v, 2) for v in b.max())} (planted object {found[-1]})")
    planted = [int(k) for k in np.argsort([-int((owner == k).sum()) for k in range(len(OBJECTS))], kind="stable")[:3]]
    return sizes, found, planted


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
