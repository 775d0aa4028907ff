"""What changed between two scans, with a sign and a significance: M3C2 on the device.

The two scans of examples/align_scans.py: a terrain with boxes scanned twice, the second scan displaced, a box added in between.  icp brings
the second scan onto the first and transform_attribute_expr applies the transform in place, as there.  Then, instead of the unsigned
cloud-to-cloud distance: subsample_min_distance thins the first scan to core points; m3c2 (Lague, Brodu & Leroux 2013; CloudCompare's plugin)
measures, per core point, the distance between the scans along the local normal of the first scan -- normals from
NearestNeighbourIndex.with_normals, turned upwards -- with its 95 % level of detection; the significant core points are filtered out through the
device mask and grouped by euclidean_clusters.  The largest group is the new box: its bounds, the sign and the mean of its change are printed
next to what the keep-far distance mask of align_scans.py returns.  Usage:

    python examples/change_detection.py [ground points per scan]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import pasture_amd as pa
from align_scans import BOXES, NEW_BOX, ORIGIN, buffer_of, rigid, scan
from pasture_amd.algorithms import _DeviceArray, transform_attribute_expr
from pasture_amd.layout import PointAttributeDataType as T, attributes as A

RADIUS, DEPTH = 1.0, 4.0        # the cylinder: a metre around the normal, four metres to either side (the new box is three metres high)
REGISTRATION_ERROR = 0.02       # what the alignment leaves, about twice the scans' noise


def main(n_ground=200_000):
    rng = np.random.default_rng(7)
    first = scan(n_ground, (0.0, 80.0), BOXES, rng)
    second_true = scan(n_ground, (20.0, 100.0), BOXES + [NEW_BOX], rng)
    pose = rigid((0.1, -0.05, 1.0), 0.4, (0.15, -0.1, 0.05), about=ORIGIN + [50.0, 50.0, 0.0])
    second = (second_true - pose[:, 3]) @ pose[:, :3]
    a, b = buffer_of(first), buffer_of(second)
    print(f"first scan {a.len()} points, second scan {b.len()} points")

    # align the second scan to the first and apply the transform in place
    reference = pa.NearestNeighbourIndex.with_normals(a, k_nn=16)
    transform, rms, matched, steps = pa.icp(b, reference, max_distance=1.0, max_iterations=50, rms_tolerance=1e-6)
    params = _DeviceArray(b.api, T.F64, 12)
    params.buffer.set_attribute_range(params.attribute, range(0, 12), transform.reshape(12))
    transform_attribute_expr(b, A.POSITION_3D, "((p0[4 * c] * x + p0[4 * c + 1] * y) + p0[4 * c + 2] * z) + p0[4 * c + 3]", [params.ptr])
    print(f"icp: {steps} steps, rms {rms:.4f}; the second scan is within {np.abs(b.view_attribute(A.POSITION_3D) - second_true).max():.4f} of where it was taken")

    # core points: the first scan thinned to a metre; the index over the aligned second scan
    core, _ = pa.subsample_min_distance(a, 1.0, seed=1)
    compared = pa.NearestNeighbourIndex(b)
    n = core.len()
    dist, lod, mask = _DeviceArray(a.api, T.F64, n), _DeviceArray(a.api, T.F64, n), _DeviceArray(a.api, T.U8, n)
    n_significant = pa.m3c2_device(core, reference, compared, RADIUS, DEPTH, min_points=4, registration_error=REGISTRATION_ERROR, orient_up=True,
                                   distance_ptr=dist.ptr, lod_ptr=lod.ptr, significant_ptr=mask.ptr)
    d, l = dist.to_numpy(), lod.to_numpy()
    measured = ~np.isnan(d)
    print(f"m3c2: {n} core points, {int(measured.sum())} with four points of either scan in their cylinder; median |distance| {np.median(np.abs(d[measured])):.4f}, "
          f"median level of detection {np.nanmedian(l):.4f}; {n_significant} significant")

    # the significant core points, grouped
    changed = core.filter(pa.HashMapBuffer, (mask.ptr, "device"))
    labels, sizes = pa.euclidean_clusters(changed, tolerance=2.0, min_size=5)
    where = changed.view_attribute(A.POSITION_3D) - ORIGIN
    values = d[mask.to_numpy() != 0]
    found = None
    for c, size in enumerate(sizes):
        member = labels == c
        lo, hi, mean = where[member].min(axis=0), where[member].max(axis=0), values[member].mean()
        print(f"change {c}: {int(size)} core points, x {lo[0]:.1f} .. {hi[0]:.1f}, y {lo[1]:.1f} .. {hi[1]:.1f}: {'raised' if mean > 0 else 'lowered'} by {abs(mean):.2f} on average"
              f" (the new box stands at {NEW_BOX[:2]}, {NEW_BOX[2]} x {NEW_BOX[3]}, {NEW_BOX[4]} high)")
        if found is None:
            found = (lo, hi, mean)

    # what align_scans.py ends on: the points of the second scan with nothing of the first within 0.6 -- unsigned, and the whole strip the first
    # scan does not cover comes along
    far_dist, far_mask = _DeviceArray(b.api, T.F64, b.len()), _DeviceArray(b.api, T.U8, b.len())
    pa.nearest_neighbours_device(b, reference, dist_ptr=far_dist.ptr)
    pa.distance_mask(far_dist.ptr, b.len(), 0.6, True, far_mask.ptr)
    far = b.filter(pa.HashMapBuffer, (far_mask.ptr, "device"))
    print(f"keep-far distance mask: {far.len()} points of the second scan further than 0.6 from the first, no sign, no significance")
    reference.destroy()
    compared.destroy()
    return found, sizes


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
