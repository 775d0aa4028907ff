"""The definitions of include/pasture_amd.h, "Individual trees", restated in numpy: no grid, chunked all-pairs, every f64 operation on a
line of its own so that nothing can fuse.  Shared by tests/test_trees.py (CPU: the rules; GPU: the device against this, bit for bit)."""
import numpy as np

NO_TREE = np.uint32(0xFFFFFFFF)
_CHUNK = 512


def heights_of(xyz, heights=None):
    return np.asarray(xyz[:, 2] if heights is None else heights, dtype=np.float64)


def valid_points(xyz, heights=None, mask=None):
    h = heights_of(xyz, heights)
    v = np.isfinite(xyz[:, 0]) & np.isfinite(xyz[:, 1]) & np.isfinite(h)
    if mask is not None:
        v &= np.asarray(mask) != 0
    return v


def window_radius(h, window):
    a, b, r_min, r_max = (np.float64(v) for v in window)
    bh = b * h
    r = a + bh
    r = np.where(r > r_min, r, r_min)
    r = np.where(r < r_max, r, r_max)
    return r


def _d2(xi, yi, xj, yj):
    """d2[i, j] from i to j: dx = x_j - x_i, dy = y_j - y_i, dx*dx + dy*dy, each rounded once"""
    dx = xj[None, :] - xi[:, None]
    dy = yj[None, :] - yi[:, None]
    dxx = dx * dx
    dyy = dy * dy
    return dxx + dyy


def tree_tops(xyz, window, min_height, heights=None, mask=None):
    """(top mask uint8 [n], indices uint32 in tree order, n_candidates)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    h = heights_of(xyz, heights)
    with np.errstate(all="ignore"):
        cand = np.flatnonzero(valid_points(xyz, heights, mask) & (h >= np.float64(min_height)))
        x, y, hc = xyz[cand, 0], xyz[cand, 1], h[cand]
        r = window_radius(hc, window)
        r2 = r * r
        top = np.zeros(n, dtype=np.uint8)
        for c0 in range(0, len(cand), _CHUNK):
            sl = slice(c0, c0 + _CHUNK)
            d2 = _d2(x[sl], y[sl], x, y)
            inside = d2 <= r2[sl, None]
            higher = hc[None, :] > hc[sl, None]
            tie = (hc[None, :] == hc[sl, None]) & (cand[None, :] < cand[sl, None])
            dominated = (inside & (higher | tie)).any(axis=1)
            top[cand[sl][~dominated]] = 1
    return top, number_trees(top, h), len(cand)


def number_trees(top_mask, h):
    """the flagged points by descending height, ties (-0.0 == +0.0) by ascending buffer index"""
    idx = np.flatnonzero(np.asarray(top_mask) != 0)
    key = -(h[idx] + 0.0)
    return idx[np.argsort(key, kind="stable")].astype(np.uint32)


def segment_trees(xyz, top_mask, max_crown_factor, exclusion, min_height, heights=None, mask=None):
    """(tree_id uint32 [n], counts uint32 [n_trees], n_labelled, indices of the trees in tree order)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    h = heights_of(xyz, heights)
    ids = np.full(n, NO_TREE, dtype=np.uint32)
    with np.errstate(all="ignore"):
        ok = valid_points(xyz, heights, mask)
        trees = number_trees(ok & (np.asarray(top_mask) != 0), h)
        nt = len(trees)
        if nt == 0:
            return ids, np.zeros(0, dtype=np.uint32), 0, trees
        # in ascending buffer index, so that argmin's first minimum is the tie rule
        asc = np.sort(trees).astype(np.int64)
        number_of = np.empty(nt, dtype=np.uint32)
        number_of[np.searchsorted(asc, trees.astype(np.int64))] = np.arange(nt, dtype=np.uint32)
        tx, ty, H = xyz[asc, 0], xyz[asc, 1], h[asc]
        half = np.float64(0.5) * np.float64(max_crown_factor)
        rc = half * H
        rc2 = rc * rc
        floor = np.float64(exclusion) * H
        q = np.flatnonzero(ok & (h >= np.float64(min_height)))
        for c0 in range(0, len(q), _CHUNK):
            p = q[c0:c0 + _CHUNK]
            d2 = _d2(xyz[p, 0], xyz[p, 1], tx, ty)
            t = np.argmin(d2, axis=1)  # (no NaN: the coordinates are finite)
            best = d2[np.arange(len(p)), t]
            good = (best <= rc2[t]) & (h[p] >= floor[t])
            ids[p[good]] = number_of[t[good]]
    counts = np.bincount(ids[ids != NO_TREE].astype(np.int64), minlength=nt).astype(np.uint32)
    return ids, counts, int(counts.sum()), trees
