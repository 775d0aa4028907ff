"""The definition of pst_height_above_ground_device (include/pasture_amd.h, "Height above ground") restated in numpy: brute force over the full
nq x ng matrix of squared XY distances, one rounded f64 operation per line.  The tests compare the device's results with this bit for bit."""
import numpy as np


def ground_set(ground, mask=None):
    """indices of G: three finite components and a non-zero mask byte (mask None: every point)"""
    ground = np.asarray(ground, dtype=np.float64).reshape(-1, 3)
    member = np.isfinite(ground).all(axis=1)
    if mask is not None:
        member &= np.asarray(mask) != 0
    return np.flatnonzero(member)


def checked_m2(max_distance):
    """max_distance as pst_nearest_neighbours_device validates it; returns m2, rounded once"""
    m2 = np.float64(max_distance) * np.float64(max_distance)
    ok = not np.isnan(max_distance) and max_distance > 0.0 and (np.isinf(m2) or (np.isfinite(m2) and m2 >= np.finfo(np.float64).tiny))
    if not ok:
        raise ValueError("max_distance")
    return m2


def height_above_ground(query, ground, mask=None, k=1, max_distance=np.inf):
    """(hag (nq,), ground_z (nq,), n_ground, n_unresolved)"""
    query = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    ground = np.asarray(ground, dtype=np.float64).reshape(-1, 3)
    m2 = checked_m2(max_distance)
    g = ground_set(ground, mask)
    nq = len(query)
    zg = np.full(nq, np.nan)
    finite_query = np.isfinite(query).all(axis=1)
    unresolved = 0
    gx, gy, gz = ground[g, 0], ground[g, 1], ground[g, 2]
    with np.errstate(all="ignore"):
        dx = gx[None, :] - query[:, 0][:, None]
        dy = gy[None, :] - query[:, 1][:, None]
        dx2 = dx * dx
        dy2 = dy * dy
        d2 = dx2 + dy2
        for q in range(nq):
            if not finite_query[q]:
                continue
            row = d2[q]
            order = np.lexsort((g, row))  # by d2, equal d2 by the ground-buffer index
            order = order[row[order] <= m2][:k]
            if len(order) == 0:
                unresolved += 1
                continue
            w = np.float64(1.0) / row[order]
            z = gz[order]
            if not w[0] < np.inf:  # an exact hit
                zg[q] = z[0]
                continue
            num = w[0] * z[0]
            den = w[0]
            for i in range(1, len(order)):
                t = w[i] * z[i]
                num = num + t
                den = den + w[i]
            zg[q] = num / den
        hag = query[:, 2] - zg
    hag[~finite_query] = np.nan
    return hag, zg, len(g), unresolved
