"""The table of objects behind a segmentation, in ONE call on the device.

Part one: the scene of examples/dbscan_objects.py -- a tilted plane, three boxes, two thin poles, stray returns and a thread -- ->
remove_ground -> dbscan -> one segment_statistics call: box, centroid, tallest point and main direction of every object, next to the sizes the
scene was built with.  Part two: the stand of examples/tree_inventory.py -> ground -> heights above it -> tree_tops -> segment_trees -> one
segment_statistics call with those heights as the values: per tree its height (the largest height above ground among its points), the point
that carries it, and the crown spread (from the horizontal covariance).

What a lidR user writes as crown_metrics, a PCL user as compute3DCentroid + computeCovarianceMatrix per cluster, and what the other examples
do with cluster_mask -> filter -> calculate_bounds in a host loop, one object at a time.  Usage:

    python examples/object_table.py [ground points] [stand points]
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


objects_scene, stand_scene = _example("dbscan_objects"), _example("tree_inventory")
PMF = dict(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)


def objects(n_ground=200_000, verbose=False):
    say = print if verbose else (lambda *a: None)
    pts, _ = objects_scene.scene(n_ground)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    rest, _ = pa.remove_ground(cloud, pa.PmfParameters(**PMF))
    labels = _DeviceArray(rest.api, T.U32, rest.len())
    found = pa.dbscan(rest, objects_scene.EPS, objects_scene.MIN_POINTS, device_labels_ptr=labels.ptr)  # the labels never leave the device
    S = len(found.sizes)
    table = pa.segment_statistics(rest, labels.ptr, S, ("count", "bounds", "centroid", "covariance", "value_max"), return_apex=True)
    values, vectors = table.principal_axes()  # (on the host: numpy.linalg.eigh of S small matrices)
    above = rest.view_attribute(A.POSITION_3D)
    say(f"{rest.len()} points above the ground, {S} objects, {table.n_members} points in them -- one call for the whole table:")
    rows = []
    for c in range(S):
        size = table.max[c] - table.min[c]
        main = vectors[c][:, 2]  # the eigenvector of the largest eigenvalue
        built = [k for k, (cx, cy, sx, sy, h) in enumerate(objects_scene.OBJECTS) if abs(table.centroid[c][0] - cx) < sx / 2 and abs(table.centroid[c][1] - cy) < sy / 2]
        planted = objects_scene.OBJECTS[built[0]] if built else None
        say(f"  object {c}: {int(table.count[c])} points, box {size[0]:.2f} x {size[1]:.2f} x {size[2]:.2f} m"
            + (f" (built {planted[2]:.2f} x {planted[3]:.2f} x {planted[4]:.2f})" if planted else "")
            + f", centroid ({table.centroid[c][0]:.2f}, {table.centroid[c][1]:.2f}, {table.centroid[c][2]:.2f}), tallest point {table.apex[c]} at z {table.value_max[c]:.2f}, "
            f"main direction ({main[0]:+.2f}, {main[1]:+.2f}, {main[2]:+.2f})")
        assert above[table.apex[c], 2] == table.value_max[c] == table.max[c][2]
        rows.append({"count": int(table.count[c]), "size": size.tolist(), "built": list(planted[2:]) if planted else None, "main": main.tolist()})
    assert np.array_equal(table.count, found.sizes.astype(np.float64))
    return rows


def trees(n_points=60_000, seed=3, verbose=False):
    say = print if verbose else (lambda *a: None)
    pts, trunks, planted_heights = stand_scene.scene(n_points, seed)
    n = len(pts)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    pa.classify_ground(cloud, pa.PmfParameters(**PMF))
    ground, hag, ids = _DeviceArray(cloud.api, T.U8, n), _DeviceArray(cloud.api, T.F64, n), _DeviceArray(cloud.api, T.U32, n)
    pa.classification_mask(cloud, 2, ground.ptr)
    pa.height_above_ground_device(cloud, ground.ptr, k=3, hag_ptr=hag.ptr)
    tops = pa.tree_tops(cloud, window=stand_scene.WINDOW, min_height=stand_scene.MIN_HEIGHT, heights=hag.ptr)
    seg = pa.segment_trees(cloud, tops, max_crown_factor=0.6, exclusion=0.3, min_height=stand_scene.MIN_HEIGHT, heights=hag.ptr, device_tree_id_ptr=ids.ptr)
    table = pa.segment_statistics(cloud, ids.ptr, seg.n_trees, ("count", "centroid", "covariance", "value_max"), values=hag.ptr, return_apex=True)
    spread = 2.0 * np.sqrt(table.covariance[:, 0, 0] + table.covariance[:, 1, 1])  # two standard deviations of the horizontal scatter
    say(f"{n} points, {seg.n_trees} trees ({len(trunks)} planted), {table.n_members} points in their crowns -- one call for the whole inventory:")
    rows = []
    for t in range(seg.n_trees):
        if table.count[t] == 0:
            continue
        rows.append({"tree": t, "points": int(table.count[t]), "height": float(table.value_max[t]), "apex": int(table.apex[t]), "crown_spread": float(spread[t])})
        if t < 5:
            say(f"  tree {t}: {table.value_max[t]:6.2f} m above the ground at point {table.apex[t]}, {int(table.count[t])} points, "
                f"crown spread {spread[t]:.2f} m around ({table.centroid[t][0]:.1f}, {table.centroid[t][1]:.1f})")
    # a tree is numbered by the height of its top, and its top is its highest point: the two calls agree
    assert np.array_equal(table.count, seg.counts.astype(np.float64))
    return rows, tops


if __name__ == "__main__":
    objects(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000, verbose=True)
    trees(int(sys.argv[2]) if len(sys.argv) > 2 else 60_000, verbose=True)
