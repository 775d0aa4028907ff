"""Roof faces of two houses, on the device: drop the ground -> region growing -> the four roof faces, next to what DBSCAN makes of the same
cloud.

What a PCL user writes as ProgressiveMorphologicalFilter + RegionGrowing, a PDAL user as filters.pmf + filters.normal + a script.  The scene
is a gently tilted ground plane with two houses on it: four walls and a gable roof each, sampled every SPACING with a little noise.  DBSCAN
(and Euclidean clusters) group by distance alone: a house is one blob.  Region growing joins neighbours whose normals agree: the two faces of
a roof meet at the ridge at an angle, the walls meet the roof at the eaves, so every face and every wall comes back as a region of its own,
largest first -- and the four largest are the roof faces.  Usage:

    python examples/roof_planes.py [ground points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import pasture_amd as pa
from pasture_amd.layout import PointLayout, attributes as A

SPACING = 0.25
NOISE = 0.005
# centre x, centre y, length along x, width along y, height of the eaves, height of the ridge (which runs along x)
HOUSES = [(30.0, 30.0, 14.0, 8.0, 3.0, 5.5), (70.0, 28.0, 10.0, 10.0, 4.0, 7.0)]
K = 16
SMOOTHNESS_DEG = 10.0
CURVATURE = 0.03
MIN_SIZE = 100


def ground_z(x, y):
    return 0.02 * x - 0.01 * y + 1.0


def _grid(a0, a1, b0, b1):
    a, b = np.arange(a0, a1 + 1e-9, SPACING), np.arange(b0, b1 + 1e-9, SPACING)
    return [v.reshape(-1) for v in np.meshgrid(a, b, indexing="ij")]


def house(cx, cy, lx, ly, eaves, ridge):
    """(points, face of every point): faces 0 and 1 are the two roof faces, -1 the walls"""
    x0, x1, y0, y1, base = cx - lx / 2, cx + lx / 2, cy - ly / 2, cy + ly / 2, ground_z(cx, cy)
    parts, faces = [], []
    rise = (ridge - eaves) / (ly / 2)
    slope = np.hypot(1.0, rise)
    for side, (ya, sign) in enumerate(((y0, 1.0), (y1, -1.0))):  # a roof face from the eaves at ya up to the ridge, sampled every SPACING along the slope
        u, s = _grid(x0, x1, 0.0, ly / 2 * slope)
        parts.append(np.column_stack([u, ya + sign * s / slope, base + eaves + s / slope * rise]))
        faces.append(np.full(len(u), side))
    for ya in (y0, y1):  # the long walls
        u, h = _grid(x0, x1, 0.0, eaves - SPACING)
        parts.append(np.column_stack([u, np.full(len(u), ya), base + h]))
        faces.append(np.full(len(u), -1))
    for xa in (x0, x1):  # the gable walls, up to the roof line
        v, h = _grid(y0 + SPACING, y1 - SPACING, 0.0, ridge)
        keep = h <= eaves + (ly / 2 - np.abs(v - cy)) * rise - SPACING
        parts.append(np.column_stack([np.full(int(keep.sum()), xa), v[keep], base + h[keep]]))
        faces.append(np.full(int(keep.sum()), -1))
    return np.concatenate(parts), np.concatenate(faces)


def scene(n_ground, seed=7):
    """(points (n, 3) in shuffled order, planted roof face of every point: 2 * house + side, -1 for ground and walls)"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n_ground, 2)) * np.array([100.0, 60.0])
    pts, face = [np.column_stack([xy, ground_z(xy[:, 0], xy[:, 1])])], [np.full(n_ground, -1)]
    for h, spec in enumerate(HOUSES):
        p, f = house(*spec)
        pts.append(p)
        face.append(np.where(f >= 0, 2 * h + f, -1))
    pts, face = np.concatenate(pts), np.concatenate(face)
    pts = pts + rng.normal(0.0, NOISE, pts.shape)
    order = rng.permutation(len(pts))
    return pts[order], face[order]


def planted_face(pts):
    """the roof face a point lies on, from its position alone (the points come back from the ground filter in another order): -1 for none"""
    face = np.full(len(pts), -1)
    for h, (cx, cy, lx, ly, eaves, ridge) in enumerate(HOUSES):
        rise = (ridge - eaves) / (ly / 2)
        roof_z = ground_z(cx, cy) + eaves + (ly / 2 - np.abs(pts[:, 1] - cy)) * rise
        on = (np.abs(pts[:, 0] - cx) <= lx / 2 + 0.05) & (np.abs(pts[:, 1] - cy) <= ly / 2 + 0.05) & (np.abs(pts[:, 2] - roof_z) <= 0.05)
        face[on] = 2 * h + (pts[on, 1] > cy)
    return face


def main(n_ground=150_000):
    pts, _ = scene(n_ground)
    cloud = pa.HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D]))
    cloud.resize(len(pts))
    cloud.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    params = pa.PmfParameters(cell_size=1.0, max_window_size=21.0, slope=1.0, initial_distance=0.5, max_distance=1.5)
    rest, n_ground_found = pa.remove_ground(cloud, params)
    above = np.asarray(rest.view_attribute(A.POSITION_3D)).reshape(-1, 3)
    face = planted_face(above)
    print(f"{len(pts)} points, {n_ground_found} of them ground; {rest.len()} above it, {int((face >= 0).sum())} of those on the four roof faces")

    regions = pa.region_growing(rest, K, smoothness_deg=SMOOTHNESS_DEG, curvature_threshold=CURVATURE, min_size=MIN_SIZE)
    print(f"region growing (k {K}, {SMOOTHNESS_DEG} degrees, curvature {CURVATURE}, min_size {MIN_SIZE}): {len(regions.sizes)} regions of "
          f"{regions.sizes.tolist()} points, {regions.n_smooth} smooth points, {regions.n_labelled} labelled")
    held = []
    for c in range(min(len(regions.sizes), 4)):
        inside = regions.labels == c
        faces = [f for f in range(4) if 2 * int((inside & (face == f)).sum()) > int((face == f).sum())]
        purity = float((face[inside] == faces[0]).mean()) if len(faces) == 1 else 0.0
        held.append(faces)
        print(f"  region {c}: {regions.sizes[c]} points, roof faces {faces}, {100.0 * purity:.1f} % of its points on that face")

    eps = 2.0 * SPACING
    blobs = pa.dbscan(rest, eps, 8)
    blob_faces = [[f for f in range(4) if 2 * int(((blobs.labels == c) & (face == f)).sum()) > int((face == f).sum())] for c in range(min(len(blobs.sizes), 4))]
    print(f"DBSCAN (eps {eps}, min_points 8): {len(blobs.sizes)} clusters of {blobs.sizes[:8].tolist()} points; the largest hold roof faces {blob_faces[:2]}")

    # the four roof faces, extracted on the device (labels and mask never leave it)
    roofs, _ = pa.extract_regions(rest, K, first_region=0, region_count=4, smoothness_deg=SMOOTHNESS_DEG, curvature_threshold=CURVATURE, min_size=MIN_SIZE)
    print(f"{roofs.len()} points on the four largest regions")
    return {"region_faces": held, "region_sizes": regions.sizes.tolist(), "dbscan_faces": blob_faces, "dbscan_sizes": blobs.sizes.tolist(), "roof_points": roofs.len(),
            "planted": [int((face == f).sum()) for f in range(4)]}


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 150_000)
