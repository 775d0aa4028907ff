"""A tree inventory on the device: rolling terrain under a stand of paraboloid crowns, and two boxes beside it -> progressive morphological
filter -> LAS class 2 -> height above ground -> tree tops by a local-maximum filter on those heights -> crowns after Silva et al. 2016.

What a lidR user writes as classify_ground(pmf()) + normalize_height(knnidw()) + locate_trees(lmf(ws, hmin)) + segment_trees(silva2016()),
and a PDAL user as filters.pmf + filters.hag_nn + filters.litree.  Prints the trees found next to the trees planted, the height and the
number of points of the five tallest, what the height floor and the window make of the boxes, and what DBSCAN makes of the same canopy:
clusters by density, which are not trees.  Only the inventory leaves the device.  Usage:

    python examples/tree_inventory.py [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

STAND = 60.0                     # metres: the stand is STAND x STAND, the boxes stand in a strip of 30 m beside it
PITCH = 10.0                     # one tree per PITCH x PITCH, jittered by +-1 m
BOXES = ((68.0, 10.0, 8.0, 6.0),  # (x0, y0, side, roof height): a shed the height floor cannot remove ...
         (70.0, 35.0, 6.0, 1.5))  # ... and a container below it
WINDOW = (3.0, 0.2, 2.0, 10.0)   # lidR's ws as a function of height, DIAMETERS: 3 + 0.2 h clamped to [2, 10]
MIN_HEIGHT = 2.0


def terrain(x, y):
    return 0.02 * x + 1.5 * np.sin(x / 15.0) * np.cos(y / 18.0)


def scene(n_points, seed):
    """(points, trunks, tree heights): one return per place -- the crown where there is one, else the roof of a box, else the ground"""
    rng = np.random.default_rng(seed)
    k = int(STAND // PITCH)
    gx, gy = np.meshgrid((np.arange(k) + 0.5) * PITCH, (np.arange(k) + 0.5) * PITCH)
    trunks = np.column_stack([gx.ravel(), gy.ravel()]) + rng.uniform(-1.0, 1.0, (k * k, 2))
    heights = rng.uniform(8.0, 20.0, k * k)
    xy = rng.random((n_points, 2)) * np.array([STAND + 30.0, STAND])
    xy[:k * k] = trunks  # a return from every apex
    above = rng.random(n_points) * 0.05
    for c0 in range(0, n_points, 20000):
        sl = slice(c0, c0 + 20000)
        d2 = ((xy[sl, None, :] - trunks[None, :, :]) ** 2).sum(axis=2)
        crown = heights[None, :] * (1.0 - d2 / (0.25 * heights[None, :]) ** 2)  # crown radius: a quarter of the height
        above[sl] = np.maximum(above[sl], crown.max(axis=1))
    for x0, y0, side, roof in BOXES:
        inside = (xy[:, 0] >= x0) & (xy[:, 0] <= x0 + side) & (xy[:, 1] >= y0) & (xy[:, 1] <= y0 + side)
        above[inside] = roof + rng.normal(0.0, 0.02, int(inside.sum()))
    order = rng.permutation(n_points)
    return np.column_stack([xy, terrain(xy[:, 0], xy[:, 1]) + above])[order], trunks, heights


def over_a_box(xy):
    hit = np.zeros(len(xy), dtype=bool)
    for x0, y0, side, _ in BOXES:
        hit |= (xy[:, 0] >= x0) & (xy[:, 0] <= x0 + side) & (xy[:, 1] >= y0) & (xy[:, 1] <= y0 + side)
    return hit


def inventory(n_points=60_000, seed=3, verbose=False):
    say = print if verbose else (lambda *a: None)
    pts, trunks, planted_heights = scene(n_points, seed)
    n = len(pts)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)

    # 1. the ground, 2. every point's height above it: a device column that never leaves the device
    n_ground = pa.classify_ground(cloud, pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2))
    ground, hag = _DeviceArray(cloud.api, T.U8, n), _DeviceArray(cloud.api, T.F64, n)
    pa.classification_mask(cloud, 2, ground.ptr)
    pa.height_above_ground_device(cloud, ground.ptr, k=3, hag_ptr=hag.ptr)
    say(f"{n} points, {n_ground} on the ground")

    # 3. the tops: local maxima of the height above ground in a window that grows with it
    tops = pa.tree_tops(cloud, window=WINDOW, min_height=MIN_HEIGHT, heights=hag.ptr)
    on_box = over_a_box(pts[tops.indices.astype(np.int64), :2])
    found = int((~on_box).sum())
    say(f"trees planted {len(trunks)}, tops found in the stand {found}; tops on the boxes {int(on_box.sum())} "
        f"(the {BOXES[1][3]} m container is under the floor of {MIN_HEIGHT} m; the flat roof of the {BOXES[0][3]} m shed is wider than the window and keeps a few)")
    small = pa.tree_tops(cloud, window=1.0, min_height=MIN_HEIGHT, heights=hag.ptr)
    small_on_box = int(over_a_box(pts[small.indices.astype(np.int64), :2]).sum())
    say(f"with a fixed window of 1 m: {small.n_tops} tops, {small_on_box} of them on the shed's roof -- the window is what tells a crown from noise")

    # 4. the crowns: every point at or above the floor goes to its nearest top if it lies within that tree's crown
    seg = pa.segment_trees(cloud, tops, max_crown_factor=0.6, exclusion=0.3, min_height=MIN_HEIGHT, heights=hag.ptr)
    tallest = [(float(tops.heights[t]), int(seg.counts[t])) for t in range(min(5, seg.n_trees))]
    say(f"{seg.n_labelled} points in {seg.n_trees} crowns; the five tallest (tree 0 first):")
    for t, (h, c) in enumerate(tallest):
        say(f"  tree {t}: {h:6.2f} m above the ground, {c} points")
    tree0 = pa.extract_tree(cloud, seg, first=0, count=1)
    assert tree0.len() == (tallest[0][1] if tallest else 0)

    # 5. the same canopy through DBSCAN: the points at or above the floor, clustered by density alone
    high = cloud.filter(pa.HashMapBuffer, hag.to_numpy() >= MIN_HEIGHT)
    blobs = pa.dbscan(high, eps=1.0, min_points=5)
    say(f"DBSCAN (eps 1 m, 5 points) on the {high.len()} points at or above {MIN_HEIGHT} m: {len(blobs.sizes)} clusters, the largest of {int(blobs.sizes.max())} points "
        f"-- density alone splits the steep flanks of a crown and joins crowns that touch: it does not count trees")
    return {"planted": len(trunks), "found": found, "tops_on_boxes": int(on_box.sum()), "boxes_found_with_a_small_window": small_on_box, "tallest": tallest,
            "counts": seg.counts.tolist(), "n_labelled": seg.n_labelled, "n_trees": seg.n_trees, "dbscan_clusters": len(blobs.sizes), "n_points": n}


if __name__ == "__main__":
    inventory(int(sys.argv[1]) if len(sys.argv) > 1 else 60_000, verbose=True)
