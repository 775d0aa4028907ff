"""Ground-plane extraction on the device: synthetic terrain -> ransac_plane -> inlier mask -> filter_into -> bounds of ground and of the rest.

What a pasture user writes with ransac_plane_serial and HashMapBuffer::filter_into, with every per-point loop on the MI355X: the positions are
scored against all hypotheses in one pass, the inlier mask is written in device memory and drives the compaction without leaving it.  Usage:

    python examples/ground_plane.py [points] [iterations]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A


def terrain(n, seed=7):
    """A tilted plane z = 0.05 x - 0.02 y + 3 with 2 cm of noise (80 % of the points) and a box of clutter above it."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 200.0
    ground = rng.random(n) < 0.8
    z = np.where(ground, 0.05 * xy[:, 0] - 0.02 * xy[:, 1] + 3.0 + rng.normal(0.0, 0.02, n), 4.0 + rng.random(n) * 30.0)
    return np.column_stack([xy, z]), ground


def main(n=200_000, iterations=100, threshold=0.1):
    pts, is_ground = terrain(n)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(n)
    cloud.set_attribute_range(A.POSITION_3D, range(0, n), pts)

    plane, indices = pa.ransac_plane(cloud, threshold, iterations, seed=1)
    norm = np.sqrt(plane.a * plane.a + plane.b * plane.b + plane.c * plane.c)
    print(f"{n} points, {iterations} hypotheses: plane ({plane.a / norm:+.4f}, {plane.b / norm:+.4f}, {plane.c / norm:+.4f}, {plane.d / norm:+.4f}) "
          f"with {plane.ranking} inliers ({int(is_ground.sum())} points were generated on the ground)")

    # the predicate as a byte mask in device memory; its complement for the rest
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    pa.plane_inlier_mask(cloud, plane, threshold, mask.data_ptr())
    pa.product_api().stream_synchronize()
    rest_mask = 1 - mask
    ground = pa.HashMapBuffer.new_from_layout(cloud.point_layout())
    ground.resize(plane.ranking)
    rest = pa.HashMapBuffer.new_from_layout(cloud.point_layout())
    rest.resize(n - plane.ranking)
    assert cloud.filter_into(ground, (mask.data_ptr(), "device"), plane.ranking) == plane.ranking == len(indices)
    assert cloud.filter_into(rest, (rest_mask.data_ptr(), "device"), n - plane.ranking) == n - plane.ranking
    gb, rb = pa.calculate_bounds(ground), pa.calculate_bounds(rest)
    print("ground bounds:", gb.min(), gb.max())
    if rb is not None:
        print("rest bounds:  ", rb.min(), rb.max())
    return plane, ground.len(), rest.len()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
