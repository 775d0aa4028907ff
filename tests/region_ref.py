"""Region growing restated in numpy (the definition of include/pasture_amd.h, "Region growing").

Inputs: neighbour lists knn (n, k), normals (n, 3), an optional curvature (n,), positions (n, 3) -- read only when max_distance is finite.
  valid   all three components of the normal are finite
  smooth  valid and curvature <= curvature_threshold (a NaN compares false; no curvature: every valid point)
  slot    slot t of i names j and counts iff j < n, j != i, j is valid and (max_distance == +inf or d <= max_distance),
          d = sqrt((dx*dx + dy*dy) + dz*dz), dx = pj.x - pi.x
  agree   fabs((ni.x*nj.x + ni.y*nj.y) + ni.z*nj.z) >= min_abs_cos
  region  a connected component of the graph on the smooth points with an edge {i, j} iff both are smooth, agree and one has the other in a
          counting slot
  rim     a valid point that is not smooth joins the region of its first slot that counts, names a smooth point and agrees
Every operation is one rounded f64 operation: numpy evaluates the expressions exactly so.  The size filter and the numbering are the clusters'
(cluster_ref.label_components), with the smallest member taken over smooth and rim members alike."""
import numpy as np

from cluster_ref import NONE, label_components, union_find

INF = float("inf")


def slot_hits(knn, normals, curvature=None, positions=None, min_abs_cos=1.0, curvature_threshold=INF, max_distance=INF):
    """(valid (n,), smooth (n,), j (n, k) int64, hit (n, k)): hit[i][t] iff slot t of i counts, names a SMOOTH point and agrees with it"""
    knn = np.asarray(knn)
    n, k = knn.shape
    normals = np.asarray(normals, dtype=np.float64).reshape(n, 3)
    j = knn.astype(np.int64) & 0xFFFFFFFF  # -1 is the 0xFFFFFFFF padding
    valid = np.isfinite(normals).all(axis=1)
    with np.errstate(all="ignore"):
        smooth = valid & (np.asarray(curvature, dtype=np.float64) <= curvature_threshold) if curvature is not None else valid.copy()
        in_range = j < n
        jj = np.where(in_range, j, 0)
        counts = in_range & (jj != np.arange(n)[:, None]) & valid[jj]
        if max_distance != INF:
            p = np.asarray(positions, dtype=np.float64).reshape(n, 3)
            dx, dy, dz = p[jj, 0] - p[:, None, 0], p[jj, 1] - p[:, None, 1], p[jj, 2] - p[:, None, 2]
            counts &= np.sqrt((dx * dx + dy * dy) + dz * dz) <= max_distance
        nj = normals[jj]
        dot = (normals[:, None, 0] * nj[..., 0] + normals[:, None, 1] * nj[..., 1]) + normals[:, None, 2] * nj[..., 2]
        agree = np.abs(dot) >= min_abs_cos
    return valid, smooth, jj, counts & agree & smooth[jj]


def components(knn, normals, curvature=None, positions=None, min_abs_cos=1.0, curvature_threshold=INF, max_distance=INF):
    """(per point the smallest index of its region's members, -1 for a point in no region; smooth (n,) bool)"""
    n = len(knn)
    valid, smooth, jj, hit = slot_hits(knn, normals, curvature, positions, min_abs_cos, curvature_threshold, max_distance)
    if n == 0:
        return np.zeros(0, dtype=np.int64), smooth
    i, t = np.nonzero(hit & smooth[:, None])
    root = union_find(n, i, jj[i, t])
    comp = np.where(smooth, root, -1)
    rim = valid & ~smooth & hit.any(axis=1)
    comp[rim] = root[jj[rim, np.argmax(hit[rim], axis=1)]]  # (argmax: the FIRST slot that hits)
    # a region's id so far is its smallest SMOOTH member; a rim member may have a smaller index
    member = comp >= 0
    lowest = np.full(n, n, dtype=np.int64)
    np.minimum.at(lowest, comp[member], np.flatnonzero(member))
    comp[member] = lowest[comp[member]]
    return comp, smooth


def region_growing(knn, normals, curvature=None, positions=None, min_abs_cos=1.0, curvature_threshold=INF, max_distance=INF, min_size=1, max_size=2 ** 64 - 1):
    """(labels uint32, sizes uint64, smooth bool) of the definition"""
    comp, smooth = components(knn, normals, curvature, positions, min_abs_cos, curvature_threshold, max_distance)
    labels, sizes = label_components(comp, min_size, max_size)
    return labels, sizes, smooth


def brute_knn(points, k):
    """(n, k) int64: the k nearest neighbours of every point, itself included, by squared distance, ties by index"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    out = np.empty((n, k), dtype=np.int64)
    rows = max(1, (1 << 24) // max(n, 1))
    for i0 in range(0, n, rows):
        d = p[i0:i0 + rows, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[i0:i0 + rows] = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return out


def corner_scene(seed=0, side=40, noise=0.002):
    """Three unit faces of side x side points that meet in one corner of a cube (z = 0, y = 0 and x = 0), with Gaussian noise on every
    coordinate: (3 * side * side, 3) float64, face by face"""
    rng = np.random.default_rng(seed)
    g = (np.arange(side) + 0.5) / side
    u, v = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    zero = np.zeros_like(u)
    faces = [np.stack([u, v, zero], axis=1), np.stack([u, zero, v], axis=1), np.stack([zero, u, v], axis=1)]
    return np.concatenate(faces) + rng.normal(0.0, noise, (3 * side * side, 3))
