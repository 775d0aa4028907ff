"""Pole detection on the device: drop the ground -> geometric features of the 16 nearest neighbours -> keep what is linear and upright ->
Euclidean clusters.

What a PDAL user writes as filters.pmf + filters.covariancefeatures + filters.range + filters.cluster.  The scene is the one of
examples/classify_ground.py: rolling terrain, three boxes and two thin poles.  A pole's neighbourhood is a line (linearity near 1) whose
smallest-eigenvalue direction is horizontal (verticality near 1); a wall or a roof is planar, a roof's edge is linear but lies flat.  The
feature columns, both masks and the compaction stay in device memory.  Usage:

    python examples/pole_detection.py [terrain points]
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray, set_u8_where
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

_spec = importlib.util.spec_from_file_location("classify_ground", os.path.join(ROOT, "examples", "classify_ground.py"))
ground_scene = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ground_scene)

K = 16
MIN_LINEARITY = 0.6     # a pole of four lines 0.25 m apart, seen over four levels: (l1 - l2) / l1 = 0.8; a wall or a roof: near 0
MIN_VERTICALITY = 0.5   # 1 - |normal.z|: 1 for a pole or a wall, 0 for a roof


def main(n_terrain=200_000):
    pts, owner = ground_scene.scene(n_terrain)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    rest, n_ground = pa.remove_ground(cloud, params)
    n = rest.len()
    print(f"{len(pts)} points, {n_ground} of them ground; {n} above it")

    # two planes in device memory, in ascending bit order: linearity, then verticality
    planes = _DeviceArray(rest.api, T.F64, 2 * n)
    pa.geometric_features_device(rest, K, ("linearity", "verticality"), planes.ptr)
    linear, lying = _DeviceArray(rest.api, T.U8, n), _DeviceArray(rest.api, T.U8, n)
    pa.distance_mask(planes.ptr, n, MIN_LINEARITY, True, linear.ptr)               # keep_far: linearity above the threshold
    pa.distance_mask(planes.ptr + 8 * n, n, MIN_VERTICALITY, False, lying.ptr)     # verticality not above its threshold ...
    set_u8_where(linear.buffer, linear.attribute, lying.ptr, 0)                    # ... is cleared from the first mask
    upright = rest.filter(pa.HashMapBuffer, (linear.ptr, "device"))
    print(f"{upright.len()} points are linear (> {MIN_LINEARITY}) and upright (verticality > {MIN_VERTICALITY})")

    tolerance = 2.0 * ground_scene.SPACING
    labels, sizes = pa.euclidean_clusters(upright, tolerance, min_size=50)
    kept = upright.view_attribute(A.POSITION_3D)[labels != pa.NO_CLUSTER]
    in_box = np.zeros(len(kept), dtype=bool)
    for cx, cy, sx, sy, _ in ground_scene.OBJECTS[:3]:
        in_box |= (np.abs(kept[:, 0] - cx) <= sx / 2 + 0.01) & (np.abs(kept[:, 1] - cy) <= sy / 2 + 0.01)
    found = 0
    for c in range(len(sizes)):
        member = upright.view_attribute(A.POSITION_3D)[labels == c]
        centre = member[:, :2].mean(axis=0)
        near = [o for o in ground_scene.OBJECTS[3:] if abs(centre[0] - o[0]) < 0.5 and abs(centre[1] - o[1]) < 0.5]
        found += len(near)
        print(f"cluster {c}: {sizes[c]} points around ({centre[0]:.2f}, {centre[1]:.2f}), z {member[:, 2].min():.2f} .. {member[:, 2].max():.2f}"
              + (" -- a pole" if near else ""))
    print(f"{found} of {len(ground_scene.OBJECTS) - 3} poles found, {int(in_box.sum())} box points among the clusters")
    return {"poles_found": found, "poles_planted": len(ground_scene.OBJECTS) - 3, "clusters": len(sizes), "box_points_kept": int(in_box.sum())}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
