"""Objects in a cloud with stray returns, on the device: drop the ground -> DBSCAN -> the objects and the noise, next to what Euclidean clusters
at the same radius make of the same cloud.

What a PDAL user writes as filters.pmf + filters.dbscan.  The scene is the one of examples/segment_objects.py -- a tilted plane, three boxes
and two thin poles -- plus a few hundred stray returns in the air and a thin thread of points (a wire, a row of birds) between the two
largest boxes.  Euclidean clusters join everything that touches: the thread makes one object of the two boxes, and every stray return is a
cluster of its own.  DBSCAN lets only points with enough neighbours carry a cluster: the thread's points have too few, so the boxes stay
apart, and the strays are noise.  Usage:

    python examples/dbscan_objects.py [ground points]
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A

_spec = importlib.util.spec_from_file_location("segment_objects", os.path.join(ROOT, "examples", "segment_objects.py"))
objects_scene = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(objects_scene)

OBJECTS, SPACING = objects_scene.OBJECTS, objects_scene.SPACING
STRAYS = 300
EPS = 2.0 * SPACING  # the radius of segment_objects.py
MIN_POINTS = 10      # a surface sampled every SPACING has 13 points within two spacings; a thread has 5


def scene(n_ground, seed=11):
    """The scene of segment_objects.py, STRAYS returns between 1.5 m and 10 m above the ground, and a thread at SPACING from the wall of the
    first box (x = 36) to the wall of the second (x = 67), 2 m above the first box's foot."""
    pts, _ = objects_scene.scene(n_ground, seed)
    rng = np.random.default_rng(seed + 1)
    xy = rng.random((STRAYS, 2)) * 100.0
    strays = np.column_stack([xy, 0.02 * xy[:, 0] - 0.01 * xy[:, 1] + 1.5 + rng.random(STRAYS) * 8.5])
    a, b = np.array([36.0 + SPACING, 30.0, 3.3]), np.array([67.0 - SPACING, 25.0, 3.3])
    steps = int(np.ceil(np.linalg.norm(b - a) / SPACING))
    thread = a + (b - a) * (np.arange(steps + 1) / steps)[:, None]
    pts = np.concatenate([pts, strays, thread])
    return pts[rng.permutation(len(pts))], len(thread)


def owner_of(pts):
    """the planted object a point stands on (by its footprint and foot height), -1 for none"""
    owner = np.full(len(pts), -1)
    for k, (cx, cy, sx, sy, h) in enumerate(OBJECTS):
        base = 0.02 * cx - 0.01 * cy + 1.0
        inside = (np.abs(pts[:, 0] - cx) <= sx / 2 + 0.01) & (np.abs(pts[:, 1] - cy) <= sy / 2 + 0.01) & (pts[:, 2] >= base - 0.01) & (pts[:, 2] <= base + h + 0.01)
        owner[inside] = k
    return owner


def main(n_ground=200_000):
    pts, n_thread = scene(n_ground)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    rest, n_ground_found = pa.remove_ground(cloud, params)
    above = rest.view_attribute(A.POSITION_3D)
    owner = owner_of(above)
    print(f"{len(pts)} points ({STRAYS} stray returns, a thread of {n_thread}), {n_ground_found} of them ground; {rest.len()} above it")

    def objects_in(labels, count):
        """for every cluster: the planted objects it holds at least half of"""
        return [[k for k in range(len(OBJECTS)) if 2 * int(((labels == c) & (owner == k)).sum()) > int((owner == k).sum())] for c in range(count)]

    result = pa.dbscan(rest, EPS, MIN_POINTS)
    noise = int((result.labels == pa.NO_CLUSTER).sum())
    print(f"DBSCAN (eps {EPS}, min_points {MIN_POINTS}): {len(result.sizes)} objects of {result.sizes.tolist()} points, "
          f"{result.n_core} core and {result.n_labelled - result.n_core} border points, {noise} noise points")
    held = objects_in(result.labels, len(result.sizes))
    for c in range(len(result.sizes)):
        print(f"  object {c}: {result.sizes[c]} points, planted objects {held[c]}")

    labels, sizes = pa.euclidean_clusters(rest, EPS)
    merged = objects_in(labels, min(len(sizes), 8))
    print(f"Euclidean clusters (tolerance {EPS}): {len(sizes)} clusters, {int((sizes == 1).sum())} of them single points; "
          f"the largest holds planted objects {merged[0] if merged else []}")

    # the objects without the noise, extracted on the device (labels and mask never leave it)
    kept, _ = pa.extract_dbscan_clusters(rest, EPS, MIN_POINTS, first_cluster=0, cluster_count=0xFFFFFFFF)
    print(f"{kept.len()} points kept")
    return {"dbscan_objects": held, "dbscan_sizes": result.sizes.tolist(), "noise": noise, "kept": kept.len(), "labelled": result.n_labelled,
            "euclidean_clusters": len(sizes), "euclidean_singles": int((sizes == 1).sum()), "euclidean_objects": merged}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
