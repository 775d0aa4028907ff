"""Two scans of one scene on the device: align the second to the first, then find what only one of them has.

A terrain with boxes is scanned twice.  The second scan overlaps the first, sees the scene from a sensor pose that is a little off (a rigid
displacement), and a box has been added in between.  icp brings the second scan onto the first (PDAL's filters.icp, PCL's
IterativeClosestPoint); the transform is applied in place through transform_attribute_expr; cloud_to_cloud_distances (CloudCompare's C2C), a
keep-far distance_mask and filter then leave the points of the second scan that the first has nothing near: the new box.  The index over
the first scan is built once and serves every ICP step and the distance query.  Usage:

    python examples/align_scans.py [ground points per scan]
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.algorithms import _DeviceArray, transform_attribute_expr
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

ORIGIN = np.array([5.0e5, 5.4e6, 100.0])  # UTM-sized coordinates
# (centre x, centre y, size x, size y, height); the last box stands in the second scan only
BOXES = [(30.0, 30.0, 12.0, 8.0, 6.0), (70.0, 25.0, 6.0, 6.0, 4.0), (50.0, 75.0, 4.0, 3.0, 2.5)]
NEW_BOX = (60.0, 50.0, 5.0, 4.0, 3.0)
SPACING = 0.25


def height(x, y):
    """Hilly ground: point-to-point ICP slides along a smooth surface, the relief (slopes up to 0.75) is what pins the scans sideways."""
    return 0.02 * x - 0.01 * y + 3.0 * np.sin(x / 4.0) * np.cos(y / 5.0)


def box_points(box):
    cx, cy, sx, sy, h = box
    base = float(height(cx, cy))
    xs = np.arange(cx - sx / 2, cx + sx / 2 + 1e-9, SPACING)
    ys = np.arange(cy - sy / 2, cy + sy / 2 + 1e-9, SPACING)
    zs = np.arange(base, base + h + 1e-9, SPACING)
    top = [(x, y, zs[-1]) for x in xs for y in ys]
    walls = [(x, y, z) for z in zs for x in xs for y in (ys[0], ys[-1])] + [(x, y, z) for z in zs for y in ys[1:-1] for x in (xs[0], xs[-1])]
    return np.array(top + walls)


def scan(n_ground, x_range, boxes, rng):
    """Ground points drawn afresh (no point of one scan is a point of the other) in x_range x [0, 100], 1 cm of noise, and the boxes."""
    x = rng.uniform(x_range[0], x_range[1], n_ground)
    y = rng.uniform(0.0, 100.0, n_ground)
    ground = np.column_stack([x, y, height(x, y) + rng.normal(0.0, 0.01, n_ground)])
    parts = [ground] + [b for b in map(box_points, boxes) if len(b)]
    pts = np.concatenate(parts)
    pts = pts[(pts[:, 0] >= x_range[0]) & (pts[:, 0] <= x_range[1])]
    return pts[rng.permutation(len(pts))] + ORIGIN


def rigid(axis, degrees, translation, about):
    a = np.asarray(axis, dtype=np.float64)
    x, y, z = a / np.linalg.norm(a)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    k = 1.0 - c
    R = np.array([[c + x * x * k, x * y * k - z * s, x * z * k + y * s], [y * x * k + z * s, c + y * y * k, y * z * k - x * s], [z * x * k - y * s, z * y * k + x * s, c + z * z * k]])
    return np.column_stack([R, about - R @ about + np.asarray(translation)])


def buffer_of(points):
    buf = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    buf.resize(len(points))
    buf.set_attribute_range(A.POSITION_3D, range(0, len(points)), points)
    return buf


def main(n_ground=200_000):
    rng = np.random.default_rng(7)
    first = scan(n_ground, (0.0, 80.0), BOXES, rng)
    second_true = scan(n_ground, (20.0, 100.0), BOXES + [NEW_BOX], rng)
    # the second scan as its sensor reports it: displaced by the inverse of `pose`
    pose = rigid((0.1, -0.05, 1.0), 0.4, (0.15, -0.1, 0.05), about=ORIGIN + [50.0, 50.0, 0.0])
    second = (second_true - pose[:, 3]) @ pose[:, :3]
    a, b = buffer_of(first), buffer_of(second)
    print(f"first scan {a.len()} points, second scan {b.len()} points, displaced by up to {np.abs(second - second_true).max():.3f}")

    index = pa.NearestNeighbourIndex(a)
    grid = index.grid()
    print(f"index: cell edge {grid['cell_edge']:.3f}, {grid['occupied_cells']} occupied cells, {grid['n_finite'] / grid['occupied_cells']:.1f} points each")

    # pairs further apart than 1 are no pairs: the parts of the second scan the first does not cover, and the new box, stay out of the fit
    transform, rms, matched, steps = pa.icp(b, index, max_distance=1.0, max_iterations=50, rms_tolerance=1e-6)
    error = np.abs(transform[:, :3] - pose[:, :3]).max()
    print(f"icp: {steps} steps, {matched} matched points, rms {rms:.4f}; rotation entries within {error:.2e} of the true pose's")

    # apply it in place, component c of every position: p0 = the 12 doubles of the transform in device memory
    params = _DeviceArray(b.api, T.F64, 12)
    params.buffer.set_attribute_range(params.attribute, range(0, 12), transform.reshape(12))
    transform_attribute_expr(b, A.POSITION_3D, "((p0[4 * c] * x + p0[4 * c + 1] * y) + p0[4 * c + 2] * z) + p0[4 * c + 3]", [params.ptr])
    residual = np.abs(b.view_attribute(A.POSITION_3D) - second_true).max()
    print(f"after alignment the second scan is within {residual:.4f} of where it was taken")

    # what is new: the points of the second scan with nothing of the first within 0.6, inside the strip both scans cover
    dist = _DeviceArray(b.api, T.F64, b.len())
    mask = _DeviceArray(b.api, T.U8, b.len())
    pa.nearest_neighbours_device(b, index, dist_ptr=dist.ptr)
    pa.distance_mask(dist.ptr, b.len(), 0.6, True, mask.ptr)
    far = b.filter(pa.HashMapBuffer, (mask.ptr, "device"))
    limit = _scalar(b.api, ORIGIN[0] + 80.0)
    overlap = far.filter_expr(pa.HashMapBuffer, "Position3D.x <= p0[0]", [limit.ptr])
    c2c = pa.cloud_to_cloud_distances(b, index)
    print(f"cloud-to-cloud: median {np.median(c2c):.3f}, {far.len()} points further than 0.6 from the first scan, {overlap.len()} of them where the scans overlap")
    bounds = pa.calculate_bounds(overlap)
    if bounds is not None:
        lo, hi = np.asarray(bounds.min()) - ORIGIN, np.asarray(bounds.max()) - ORIGIN
        print(f"the change: bounds {tuple(round(v, 2) for v in lo)} .. {tuple(round(v, 2) for v in hi)} (the new box stands at {NEW_BOX[:2]}, {NEW_BOX[2]} x {NEW_BOX[3]} x {NEW_BOX[4]})")
    index.destroy()
    found = overlap.view_attribute(A.POSITION_3D) - ORIGIN
    return residual, found


def _scalar(api, value):
    d = _DeviceArray(api, T.F64, 1)
    d.buffer.set_attribute_range(d.attribute, range(0, 1), np.array([value]))
    return d


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
