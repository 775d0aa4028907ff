"""Polygon crop and overlay on the device: the scene of examples/classify_ground.py -> progressive morphological filter -> crop to an L-shaped
parcel with a hole -> overlay two building footprints into Classification as class 6 -> Euclidean clusters of what stands inside the parcel.

What a PDAL user writes as filters.pmf + filters.crop (polygon) + filters.overlay + filters.cluster, a lidR user as clip_roi and
merge_spatial.  The polygons never leave the caller's arrays as anything but arrays: no WKT, no files.  Usage:

    python examples/crop_polygon.py [terrain points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A

from classify_ground import OBJECTS, SPACING, scene

# the parcel: an L (the north-east quarter is someone else's) with a pond cut out of it -- the second ring is a hole by the even-odd rule
PARCEL = [np.array([[5.0, 5.0], [95.0, 5.0], [95.0, 55.0], [60.0, 55.0], [60.0, 95.0], [5.0, 95.0]]),
          np.array([[40.0, 50.0], [48.0, 48.0], [52.0, 56.0], [44.0, 60.0]])]


def footprint(obj, margin=0.5):
    cx, cy, sx, sy, _ = obj
    x0, x1, y0, y1 = cx - sx / 2 - margin, cx + sx / 2 + margin, cy - sy / 2 - margin, cy + sy / 2 + margin
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])


def in_parcel(x, y):
    """the parcel by plain comparisons, for the check of the crop below (the pond is a convex quadrilateral)"""
    inside_l = (x >= 5.0) & (x < 95.0) & (y >= 5.0) & (y < 95.0) & ~((x >= 60.0) & (y >= 55.0))
    pond = PARCEL[1]
    a, b = pond, np.roll(pond, -1, axis=0)
    sides = [(b[k, 0] - a[k, 0]) * (y - a[k, 1]) - (x - a[k, 0]) * (b[k, 1] - a[k, 1]) for k in range(4)]
    return inside_l & ~np.all([s > 0 for s in sides], axis=0)


def main(n_terrain=200_000):
    pts, owner = scene(n_terrain)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    n_ground = pa.classify_ground(cloud, params)
    print(f"{len(pts)} points, {n_ground} of them ground (class 2)")

    # the crop: one set, indexed once, used for the mask's count and for the compaction
    parcel = pa.PolygonSet([PARCEL])
    print(f"the parcel: {parcel.info}")
    inside, n_inside = pa.crop(cloud, parcel)
    outside, n_outside = pa.crop(cloud, parcel, outside=True)
    expected = in_parcel(pts[:, 0], pts[:, 1])
    near_edge = int((expected != (pa.points_in_polygons(cloud, parcel) != pa.NO_POLYGON)).sum())  # only points within rounding of a slanted pond edge could differ
    print(f"{n_inside} points inside the parcel, {n_outside} outside; plain comparisons say {int(expected.sum())} ({near_edge} differ)")
    parcel.destroy()

    # the overlay: the two largest buildings' footprints become class 6 (building) -- inside the cropped cloud, in place, on the device
    footprints = [footprint(OBJECTS[0]), footprint(OBJECTS[1])]
    n_building = pa.overlay(inside, A.CLASSIFICATION, footprints, [6, 6])
    classes = inside.view_attribute(A.CLASSIFICATION)
    print(f"{n_building} points fall in the two footprints: classes now {dict(zip(*[v.tolist() for v in np.unique(classes, return_counts=True)]))}")

    # what stands inside the parcel: drop the ground, cluster the rest
    standing = inside.filter(pa.HashMapBuffer, classes != 2)
    labels, sizes = pa.euclidean_clusters(standing, 2.0 * SPACING, min_size=50)
    print(f"{standing.len()} points above the ground inside the parcel: {len(sizes)} objects of {sizes.tolist()} points")
    return {"inside": n_inside, "outside": n_outside, "expected_inside": int(expected.sum()), "differ": near_edge, "building": n_building, "clusters": len(sizes)}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
