"""Ground classification on the device: rolling terrain with boxes and poles on it -> progressive morphological filter -> LAS class 2 ->
drop the ground -> Euclidean clusters.

What a PDAL user writes as filters.pmf + filters.range + filters.cluster.  The terrain is NOT a plane, so the plane fit the other examples take
the ground from (examples/ground_plane.py, examples/segment_objects.py) leaves most of it standing; the count is printed for contrast.  Usage:

    python examples/classify_ground.py [terrain points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A

# (centre x, centre y, size x, size y, height): three boxes of decreasing size and two thin poles
OBJECTS = [(30.0, 30.0, 12.0, 8.0, 6.0), (70.0, 25.0, 6.0, 6.0, 4.0), (50.0, 75.0, 4.0, 3.0, 2.5), (15.0, 80.0, 0.3, 0.3, 8.0), (85.0, 85.0, 0.3, 0.3, 6.0)]
SPACING = 0.25  # point spacing on the objects' surfaces
CLEAR = 2.0     # the walls end this far above the terrain


def height(x, y):
    return 0.02 * x + 1.5 * np.sin(x / 15.0) * np.cos(y / 18.0)


def scene(n_terrain, seed=11):
    """100 m x 100 m of rolling terrain with 2 cm of noise -- none of it under the boxes, which a scanner does not see -- and the objects' tops and
    walls sampled every SPACING.  Returns (points, object number per point or -1 for the terrain), shuffled."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n_terrain, 2)) * 100.0
    for cx, cy, sx, sy, _ in OBJECTS[:3]:
        xy = xy[~((np.abs(xy[:, 0] - cx) < sx / 2) & (np.abs(xy[:, 1] - cy) < sy / 2))]
    terrain = np.column_stack([xy, height(xy[:, 0], xy[:, 1]) + rng.normal(0.0, 0.02, len(xy))])
    parts, owner = [terrain], [np.full(len(terrain), -1)]
    for k, (cx, cy, sx, sy, h) in enumerate(OBJECTS):
        top_z = height(cx, cy) + CLEAR + h
        xs = np.arange(cx - sx / 2, cx + sx / 2 + 1e-9, SPACING)
        ys = np.arange(cy - sy / 2, cy + sy / 2 + 1e-9, SPACING)
        top = [(x, y, top_z) for x in xs for y in ys]
        rim = [(x, y) for x in xs for y in (ys[0], ys[-1])] + [(x, y) for y in ys[1:-1] for x in (xs[0], xs[-1])]
        walls = [(x, y, z) for x, y in rim for z in np.arange(height(x, y) + CLEAR, top_z, SPACING)]
        obj = np.array(top + walls)
        parts.append(obj)
        owner.append(np.full(len(obj), k))
    pts, owner = np.concatenate(parts), np.concatenate(owner)
    order = rng.permutation(len(pts))
    return pts[order], owner[order]


def main(n_terrain=200_000):
    pts, owner = scene(n_terrain)
    terrain = owner < 0
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    print(f"{len(pts)} points: {int(terrain.sum())} on the terrain, {int((~terrain).sum())} on {len(OBJECTS)} objects")

    # the filter: 1 m cells, windows of 3, 5, 9 and 17 cells -- no box holds the last one -- and thresholds below the walls' lower end
    params = pa.PmfParameters(cell_size=1.0, max_window_size=17.0, slope=1.0, initial_distance=0.5, max_distance=1.2)
    half_widths, thresholds = pa.pmf_schedule(params)
    print(f"windows of half-width {half_widths.tolist()} cells, thresholds {thresholds.tolist()}")
    n_ground = pa.classify_ground(cloud, params)  # LAS class 2, written on the device; every other point keeps its class
    classes = cloud.view_attribute(A.CLASSIFICATION)
    is_ground = classes == 2
    recall = float(is_ground[terrain].mean())
    objects_as_ground = int(is_ground[~terrain].sum())
    print(f"{n_ground} ground points: {100.0 * recall:.2f} % of the terrain, {objects_as_ground} object points among them")

    # for contrast: the plane most points lie within 15 cm of, on the same cloud
    plane, inliers = pa.ransac_plane(cloud, 0.15, 256, seed=3)
    plane_left = int(terrain.sum()) - int(terrain[inliers.astype(np.int64)].sum())
    pmf_left = int((~is_ground[terrain]).sum())
    print(f"terrain points left standing: {pmf_left} by the filter, {plane_left} by a RANSAC plane ({plane.ranking} inliers)")

    # drop the ground (mask and compaction stay on the device), then clusters: closer than two spacings, at least 50 points
    rest, _ = pa.remove_ground(cloud, params)
    tolerance = 2.0 * SPACING
    labels, sizes = pa.euclidean_clusters(rest, tolerance, min_size=50)
    print(f"{rest.len()} points above the ground: {len(sizes)} objects of {sizes.tolist()} points; {int((labels == pa.NO_CLUSTER).sum())} points in none")
    largest, _ = pa.extract_clusters(rest, tolerance, min_size=50)
    b = pa.calculate_bounds(largest)
    print(f"the largest: {largest.len()} points, bounds {tuple(round(v, 2) for v in b.min())} .. {tuple(round(v, 2) for v in b.max())}")
    return {"ground_recall": recall, "objects_as_ground": objects_as_ground, "pmf_left_over": pmf_left, "plane_left_over": plane_left,
            "clusters_found": len(sizes), "objects_planted": len(OBJECTS)}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
