"""Radius neighbourhoods on the device: a point density per point, and geometric features over ALL points within a radius instead of the k
nearest.

What a PDAL user writes as filters.radialdensity, and a CloudCompare or jakteristics user as "geometric features, radius 0.5".  The scene
is the one of examples/pole_detection.py: rolling terrain, three boxes and two thin poles, with the ground removed.  The counts within 0.5 m
are the density; the neighbour lists (CSR: offsets, indices, distances, nearest first) are padded to their 16 nearest and handed to
geometric_features as its `knn`, next to the features of the plain 16 nearest neighbours.  Usage:

    python examples/radius_neighbours.py [terrain points]
"""
import importlib.util
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A

_spec = importlib.util.spec_from_file_location("classify_ground", os.path.join(ROOT, "examples", "classify_ground.py"))
ground_scene = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ground_scene)

RADIUS = 0.5
K = 16
FEATURES = ("linearity", "planarity", "scattering", "verticality")


def main(n_terrain=200_000):
    pts, owner = ground_scene.scene(n_terrain)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    rest, n_ground = pa.remove_ground(cloud, params)
    n = rest.len()
    print(f"{len(pts)} points, {n_ground} of them ground; {n} above it")

    index = pa.NearestNeighbourIndex(rest)  # built once, searched twice
    counts = pa.radius_neighbour_counts(rest, index, RADIUS)
    density = counts / (4.0 / 3.0 * math.pi * RADIUS ** 3)
    print(f"points within {RADIUS} m (the point itself included): min {counts.min()}, median {int(np.median(counts))}, max {counts.max()};"
          f" median density {np.median(density):.1f} points per cubic metre")

    lists = pa.radius_search(rest, index, RADIUS)
    index.destroy()
    assert np.array_equal(lists.counts, counts)
    i, d = lists.list(int(np.argmax(counts)))
    print(f"{len(lists.indices)} entries in all; the fullest list starts with points {i[:4]} at {np.round(d[:4], 3)} m")

    by_radius = pa.geometric_features(rest, K, FEATURES, knn=lists.to_padded(K))   # the 16 nearest of those within the radius
    by_k = pa.geometric_features(rest, K, FEATURES)                                # the 16 nearest, however far
    print(f"{'':12s} {'within ' + str(RADIUS) + ' m':>14s} {'k = ' + str(K):>14s}   (medians over the points where both are defined)")
    both = np.isfinite(by_radius["linearity"]) & np.isfinite(by_k["linearity"])
    for name in FEATURES:
        print(f"{name:12s} {np.median(by_radius[name][both]):14.3f} {np.median(by_k[name][both]):14.3f}")
    sparse = int((counts < 3).sum())
    print(f"{sparse} points have fewer than 3 points within the radius: their radius features are undefined, their k = {K} features are not")
    return {"points": n, "entries": int(len(lists.indices)), "sparse": sparse}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
