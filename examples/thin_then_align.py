"""Thin the moving scan before aligning it: the scene of align_scans.py, once as it is and once with the second scan subsampled first.

Every ICP step sends every source point through the index, so the step costs what the source has points; the fit itself needs far fewer than a
scanner delivers.  subsample_min_distance (PDAL's filters.sample, CloudCompare's "subsample by space") keeps original points of the second
scan such that no two are closer than a radius -- an even density, whatever the scanner's was -- and icp runs on those.  The transform found
on the thinned scan is then applied to ALL points of the second scan, and the residual displacement is measured on all of them.  Usage:

    python examples/thin_then_align.py [ground points per scan] [radius]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import pasture_amd as pa
from align_scans import BOXES, NEW_BOX, ORIGIN, buffer_of, rigid, scan


def align(source, index, second, second_true):
    """(steps, matched, rms, residual displacement of the WHOLE second scan under the transform found on `source`, seconds of the icp call)"""
    t0 = time.perf_counter()
    transform, rms, matched, steps = pa.icp(source, index, max_distance=1.0, max_iterations=50, rms_tolerance=1e-6)
    seconds = time.perf_counter() - t0
    moved = second @ transform[:, :3].T + transform[:, 3]
    return steps, matched, rms, float(np.abs(moved - second_true).max()), seconds


def main(n_ground=200_000, radius=0.5):
    rng = np.random.default_rng(7)
    first = scan(n_ground, (0.0, 80.0), BOXES, rng)
    second_true = scan(n_ground, (20.0, 100.0), BOXES + [NEW_BOX], rng)
    pose = rigid((0.1, -0.05, 1.0), 0.4, (0.15, -0.1, 0.05), about=ORIGIN + [50.0, 50.0, 0.0])
    second = (second_true - pose[:, 3]) @ pose[:, :3]
    a, b = buffer_of(first), buffer_of(second)
    index = pa.NearestNeighbourIndex(a)

    thin, kept = pa.subsample_min_distance(b, radius, seed=1)
    _, _, rounds = pa.poisson_disk_mask(b, radius, seed=1)
    print(f"second scan: {b.len()} points; no two closer than {radius}: {kept} points ({100.0 * kept / b.len():.1f} %), decided in {rounds} rounds")
    # the guarantee, through the library's own clustering: at tolerance = radius the thinned scan is all singletons
    _, sizes = pa.euclidean_clusters(thin, radius)
    assert len(sizes) == kept and int(sizes.max()) == 1

    rows = {}
    for name, source in (("all points", b), ("thinned", thin)):
        rows[name] = align(source, index, second, second_true)
        steps, matched, rms, residual, seconds = rows[name]
        print(f"{name:>10}: {source.len():>8} source points, {steps:>2} icp steps, {matched:>8} matched, rms {rms:.4f}, "
              f"residual displacement of the whole scan {residual:.4f}, icp call {1e3 * seconds:.1f} ms")
    index.destroy()
    displaced = float(np.abs(second - second_true).max())
    print(f"(before alignment the scan was displaced by up to {displaced:.4f})")
    return kept, displaced, rows["all points"], rows["thinned"]


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000, float(sys.argv[2]) if len(sys.argv) > 2 else 0.5)
