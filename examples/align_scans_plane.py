"""The scene of align_scans.py aligned by point-to-plane ICP, next to point-to-point on the same index.

Scans are surfaces.  Point-to-point ICP pulls every point of the second scan towards its nearest neighbour in the first, which on a surface is
a fraction of the point spacing away whatever the offset within the surface is: it creeps.  Point-to-plane ICP (PCL's
IterativeClosestPointWithNormals, Open3D's point-to-plane estimation) only counts the distance along the first scan's normal, so the scans
are free to slide into place.  NearestNeighbourIndex.with_normals builds the index over the first scan and estimates its normals on the
device (their signs are arbitrary, which the step does not mind); icp_plane and icp then share it.  Usage:

    python examples/align_scans_plane.py [ground points per scan]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import pasture_amd as pa
from align_scans import BOXES, NEW_BOX, ORIGIN, buffer_of, rigid, scan


def displacement(transform, points, truth):
    """the largest distance between a transformed point and where it belongs"""
    moved = points @ transform[:, :3].T + transform[:, 3]
    return float(np.linalg.norm(moved - truth, axis=1).max())


def main(n_ground=200_000):
    rng = np.random.default_rng(7)
    first = scan(n_ground, (0.0, 80.0), BOXES, rng)
    second_true = scan(n_ground, (20.0, 100.0), BOXES + [NEW_BOX], rng)
    pose = rigid((0.1, -0.05, 1.0), 0.4, (0.15, -0.1, 0.05), about=ORIGIN + [50.0, 50.0, 0.0])
    second = (second_true - pose[:, 3]) @ pose[:, :3]
    a, b = buffer_of(first), buffer_of(second)
    start = displacement(np.eye(3, 4), second, second_true)
    print(f"first scan {a.len()} points, second scan {b.len()} points, displaced by up to {start:.3f}")

    index = pa.NearestNeighbourIndex.with_normals(a, k_nn=16)
    results = {}
    for name, run in (("point-to-plane", pa.icp_plane), ("point-to-point", pa.icp)):
        transform, rms, pairs, steps = run(b, index, max_distance=1.0, max_iterations=50, rms_tolerance=1e-6)
        results[name] = {"steps": steps, "rms": rms, "pairs": pairs, "residual": displacement(transform, second, second_true),
                         "rotation_error": float(np.abs(transform[:, :3] - pose[:, :3]).max())}
        r = results[name]
        print(f"{name}: {steps} steps, {pairs} pairs, rms {rms:.4f}; remaining displacement {r['residual']:.4f}, rotation entries within {r['rotation_error']:.2e}")
    index.destroy()
    return results["point-to-plane"], results["point-to-point"]


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
