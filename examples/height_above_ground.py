"""Height above ground on the device: the scene of examples/classify_ground.py -> progressive morphological filter -> LAS class 2 -> height of
every point above the ground interpolated from its 10 nearest ground points in the XY plane -> keep what stands more than 2 m high -> Euclidean
clusters, with the tallest height of each next to the height the object was built with.

What a PDAL user writes as filters.pmf + filters.hag_nn + filters.range + filters.cluster.  Nothing but the printed figures leaves the device.  Usage:

    python examples/height_above_ground.py [terrain points]
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

_spec = importlib.util.spec_from_file_location("classify_ground_scene", os.path.join(ROOT, "examples", "classify_ground.py"))
scene_module = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(scene_module)

KEEP_ABOVE = 2.0  # metres above the ground


def main(n_terrain=200_000):
    pts, owner = scene_module.scene(n_terrain)
    n = len(pts)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    n_ground = pa.classify_ground(cloud, params)

    # Classification == 2 -> ground mask -> height above ground, all in device memory
    ground, hag, tall = _DeviceArray(cloud.api, T.U8, n), _DeviceArray(cloud.api, T.F64, n), _DeviceArray(cloud.api, T.U8, n)
    pa.classification_mask(cloud, 2, ground.ptr)
    info = pa.height_above_ground_device(cloud, ground.ptr, k=10, hag_ptr=hag.ptr)
    print(f"{n} points, {n_ground} on the ground; grid of {info['dim'][0]} x {info['dim'][1]} cells of {info['cell_edge']:.3f} m, "
          f"{info['n_unresolved']} points without a height")

    # keep what stands more than KEEP_ABOVE high (a point without a height would be kept too: NOT hag <= 2), then clusters
    pa.distance_mask(hag.ptr, n, KEEP_ABOVE, True, tall.ptr)
    standing = cloud.filter(pa.HashMapBuffer, (tall.ptr, "device"))
    labels, sizes = pa.euclidean_clusters(standing, 2.0 * scene_module.SPACING, min_size=50)
    print(f"{standing.len()} points stand more than {KEEP_ABOVE} m above the ground: {len(sizes)} objects")

    # the tallest height per object, next to what the scene was built with: the walls end CLEAR above the terrain, the top h above that
    heights = hag.to_numpy()[tall.to_numpy() != 0]  # in the order of the compaction: the order of `standing`
    xy = standing.view_attribute(A.POSITION_3D)[:, :2]
    found = []
    for c in range(len(sizes)):
        members = labels == c
        centre = xy[members].mean(axis=0)
        k = int(np.argmin([np.hypot(centre[0] - o[0], centre[1] - o[1]) for o in scene_module.OBJECTS]))
        built = scene_module.CLEAR + scene_module.OBJECTS[k][4]
        tallest = float(heights[members].max())
        found.append({"object": k, "tallest": tallest, "built": built})
        print(f"  object {k} at ({centre[0]:.1f}, {centre[1]:.1f}): {int(sizes[c])} points, tallest {tallest:.2f} m above the ground; built {built:.2f} m above the terrain")
    return {"objects_planted": len(scene_module.OBJECTS), "found": found, "n_unresolved": info["n_unresolved"], "n_ground": n_ground}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
