"""A numpy restatement of pst_rasterize_quantiles and pst_segment_quantiles, written from the text of include/pasture_amd.h ("Quantiles").

A group's values are sorted by the u64 key that orders the doubles with -0.0 below +0.0 -- not with np.sort, which treats the two zeros as
equal.  h, lo and g are numpy float64 scalars, so every operation rounds once, like the kernels (compiled without contraction)."""
import numpy as np

from raster_ref import auto_grid
from segments_ref import members_of

METHODS = {"linear": 0, "lower": 1, "higher": 2}
NAN_BITS = np.uint64(0x7FF8000000000000)
NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def bits(a):
    """the u64 view results are compared through: NaNs as bits, -0.0 apart from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ordered(a):
    """the order-preserving keys of doubles: -0.0 below +0.0"""
    u = bits(a)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(0x8000000000000000))


def sort_values(values):
    """s_0 .. s_(m-1): ascending by the ordered key"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    return v[np.argsort(ordered(v), kind="stable")]


def quantile(s, p, method="linear"):
    """the quantile of the sorted values s (m >= 1) at probability p"""
    m = len(s)
    with np.errstate(all="ignore"):
        h = np.float64(m - 1) * np.float64(p)
        lo = int(np.floor(h))
        g = h - np.float64(lo)
        if g == 0.0 or method == "lower":
            return s[lo]
        if method == "higher":
            return s[lo + 1]
        return s[lo] + g * (s[lo + 1] - s[lo])


def group_planes(group, values, n_groups, probs=(), thresholds=(), method="linear"):
    """the core: group (int per member, all < n_groups) and values (float64 per member) -> [1 + P + T][n_groups]"""
    group = np.asarray(group, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    P, T = len(probs), len(thresholds)
    out = np.empty((1 + P + T, n_groups), dtype=np.float64)
    out[0] = 0.0
    out[1:1 + P] = NAN
    out[1 + P:] = 0.0
    order = np.lexsort((ordered(values), group))  # by group, then by key
    g_sorted, v_sorted = group[order], values[order]
    heads = np.flatnonzero(np.concatenate([[True], g_sorted[1:] != g_sorted[:-1]])) if len(order) else np.zeros(0, dtype=np.int64)
    ends = np.concatenate([heads[1:], [len(order)]]) if len(order) else heads
    for a, b in zip(heads, ends):
        c, s = g_sorted[a], v_sorted[a:b]
        out[0, c] = np.float64(b - a)
        for i, p in enumerate(probs):
            out[1 + i, c] = quantile(s, p, method)
        for i, t in enumerate(thresholds):
            out[1 + P + i, c] = np.float64(np.count_nonzero(s > np.float64(t)))  # compared as doubles
    return out


def segment_quantiles(pts, labels, n_segments, probs=(), thresholds=(), method="linear", values=None, mask=None):
    """-> ([1 + P + T][S], n_members)"""
    ok, v = members_of(pts, labels, n_segments, values, mask)
    labels = np.asarray(labels).astype(np.int64) & 0xFFFFFFFF
    out = group_planes(labels[ok], v[ok], int(n_segments), probs, thresholds, method)
    return out, int(ok.sum())


def rasterize_quantiles(pts, cell, probs=(), thresholds=(), method="linear", values=None, mask=None, origin=None, dim=None):
    """-> ([1 + P + T][rows * cols], n_members, (x0, y0, cols, rows)); the member test and the cell are pst_rasterize's"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cell = np.float64(cell)
    if origin is None:
        x0, y0, cols, rows = auto_grid(pts, cell)
    else:
        (x0, y0), (cols, rows) = origin, dim
    x0, y0 = np.float64(x0), np.float64(y0)
    v = pts[:, 2] if values is None else np.asarray(values, dtype=np.float64)
    with np.errstate(all="ignore"):
        qx, qy = (pts[:, 0] - x0) / cell, (pts[:, 1] - y0) / cell
        ok = np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1]) & np.isfinite(v)
        if mask is not None:
            ok &= np.asarray(mask) != 0
        ok &= (qx >= 0.0) & (qx < float(cols)) & (qy >= 0.0) & (qy < float(rows))
    group = qy[ok].astype(np.int64) * cols + qx[ok].astype(np.int64)
    out = group_planes(group, v[ok], cols * rows, probs, thresholds, method)
    return out, int(ok.sum()), (float(x0), float(y0), cols, rows)
