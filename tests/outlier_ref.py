"""numpy restatement of pst_knn_search_device / pst_statistical_outlier_mask / pst_radius_outlier_mask (include/pasture_amd.h).

Brute force in chunks of queries.  d2 = (dx*dx + dy*dy) + dz*dz with dx = p.x - q.x (neighbour minus query), every operation one rounded f64
operation; a NaN d2 counts as +inf for the ORDER; slots in ascending (d2, index); the distance of a slot is np.sqrt of its own d2 (a NaN stays
a NaN: what IEEE arithmetic gives); a padded slot (index -1) is +inf.  dbar adds the columns 1 .. mean_k one at a time; the statistics use
math.fsum (the correctly rounded sum) and are what the device's fixed-shape sums are measured against."""
import math

import numpy as np


def knn(pts, k, queries=None, chunk=256):
    """(indices (q, k) int64 with -1 padding, distances (q, k) float64) of `queries` (indices into pts; default: every point)."""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    n = pts.shape[0]
    queries = np.arange(n) if queries is None else np.asarray(queries, dtype=np.int64)
    idx = np.full((len(queries), k), -1, dtype=np.int64)
    dist = np.full((len(queries), k), np.inf, dtype=np.float64)
    m = min(n, k)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, len(queries), chunk):
            q = pts[queries[c0:c0 + chunk]]
            dx = pts[None, :, 0] - q[:, None, 0]
            dy = pts[None, :, 1] - q[:, None, 1]
            dz = pts[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            key = np.where(np.isnan(d2), np.inf, d2)
            # the m-th smallest key of each row; every candidate is <= it, and taking them in index order and sorting them stably by key is
            # the stable sort of the whole row by (key, index), cut at m
            kth = np.partition(key, m - 1, axis=1)[:, m - 1]
            for r in range(q.shape[0]):
                cand = np.flatnonzero(key[r] <= kth[r])
                order = cand[np.argsort(key[r, cand], kind="stable")][:m]
                idx[c0 + r, :m] = order
                dist[c0 + r, :m] = np.sqrt(d2[r, order])
    return idx, dist


def mean_distances(dist, mean_k):
    """dbar = (d[1] + d[2] + ... + d[mean_k]) / mean_k, the columns added one at a time, left to right."""
    with np.errstate(invalid="ignore"):
        s = dist[:, 1].copy()
        for t in range(2, mean_k + 1):
            s = s + dist[:, t]
        return s / np.float64(mean_k)


def statistics(dbar, stddev_mult):
    """(mean, stddev, threshold, m) over the finite dbar with correctly rounded sums; two passes; stddev = 0 when m < 2."""
    f = dbar[np.isfinite(dbar)]
    m = len(f)
    mean = math.fsum(f) / m if m else float("nan")
    stddev = math.sqrt(math.fsum((f - mean) * (f - mean)) / (m - 1)) if m >= 2 else 0.0
    return mean, stddev, mean + stddev_mult * stddev, m


def statistical_mask(dbar, threshold):
    with np.errstate(invalid="ignore"):
        return (np.isfinite(dbar) & (dbar <= threshold)).astype(np.uint8)


def radius_mask(dist, radius, min_neighbours):
    """dist: at least min_neighbours + 1 columns.  A padded slot (+inf) or a NaN compares false."""
    with np.errstate(invalid="ignore"):
        return (dist[:, min_neighbours] <= radius).astype(np.uint8)
