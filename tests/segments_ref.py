"""A numpy restatement of pst_segment_statistics, written from the text of include/pasture_amd.h ("Segment statistics").

Every sum is the fixed tree T of the header.  numpy adds float64 arrays element by element with one IEEE rounding per addition, like the
kernels (compiled without contraction), so slicing the groups and adding the slices IS the definition; np.sum (pairwise) is never used."""
import numpy as np

from raster_ref import wide_values  # noqa: F401  (values over 30 decades with mixed signs: their sum shows the order of its additions)

GROUP = 256  # PST_SEGMENT_GROUP: part of the definition
STATS = ("count", "bounds", "centroid", "covariance", "value_min", "value_max", "value_mean", "value_variance")  # ascending bit order
BITS = {s: 1 << i for i, s in enumerate(STATS)}
PLANES = {"count": 1, "bounds": 6, "centroid": 3, "covariance": 6, "value_min": 1, "value_max": 1, "value_mean": 1, "value_variance": 1}
NAN_BITS = np.uint64(0x7FF8000000000000)
NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]
NO_APEX = 0xFFFFFFFF


def bits(a):
    """the u64 view results are compared through: NaNs as bits, -0.0 apart from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ordered(a):
    """the order-preserving keys of doubles: -0.0 below +0.0"""
    u = bits(a)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(0x8000000000000000))


def tree_level(values):
    """one level of T: the partials of the groups of 256, the last one padded with -0.0"""
    v = np.asarray(values, dtype=np.float64)
    groups = -(-len(v) // GROUP)
    g = np.full(groups * GROUP, -0.0)
    g[:len(v)] = v
    g = g.reshape(groups, GROUP)
    with np.errstate(all="ignore"):
        r = ((g[:, 0:64] + g[:, 64:128]) + g[:, 128:192]) + g[:, 192:256]
        for h in (32, 16, 8, 4, 2, 1):
            r = r[:, :h] + r[:, h:2 * h]
    return r[:, 0]


def tree_sum(values):
    """T: levels until one value is left; a sequence of one element is that element"""
    v = np.asarray(values, dtype=np.float64)
    assert len(v) > 0
    while len(v) > 1:
        v = tree_level(v)
    return v[0]


def plain_sum(values):
    s = np.float64(values[0])
    for v in values[1:]:
        s = s + np.float64(v)
    return s


def members_of(pts, labels, n_segments, values=None, mask=None):
    """the member test of the header -> (bool per point, the values)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels).astype(np.int64) & 0xFFFFFFFF
    v = pts[:, 2] if values is None else np.asarray(values, dtype=np.float64)
    ok = (labels < n_segments) & np.isfinite(pts).all(axis=1) & np.isfinite(v)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok, v


def statistics(pts, labels, n_segments, stats=STATS, values=None, mask=None):
    """-> ({name: [planes][S] float64}, apex uint32 [S], n_members): every statistic of STATS in `stats`, in the plane layout of the C ABI"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    S = int(n_segments)
    labels = np.asarray(labels).astype(np.int64) & 0xFFFFFFFF
    ok, v = members_of(pts, labels, S, values, mask)
    idx = np.flatnonzero(ok)
    idx = idx[np.argsort(labels[idx], kind="stable")]  # by segment, ascending buffer index within one
    counts = np.bincount(labels[idx], minlength=S)[:S] if len(idx) else np.zeros(S, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)])
    out = {s: np.full((PLANES[s], S), NAN, dtype=np.float64) for s in STATS}
    out["count"][0] = counts.astype(np.float64)
    apex = np.full(S, NO_APEX, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for s in np.flatnonzero(counts):
            a = idx[starts[s]:starts[s + 1]]
            m = np.float64(len(a))
            p, w = pts[a], v[a]
            for c in range(3):
                k = ordered(p[:, c])
                out["bounds"][c, s] = p[np.argmin(k), c]
                out["bounds"][3 + c, s] = p[np.argmax(k), c]
            k = ordered(w)
            out["value_min"][0, s] = w[np.argmin(k)]
            out["value_max"][0, s] = w[np.argmax(k)]
            apex[s] = a[np.argmax(k)]  # (argmax: the first of the largest, and `a` ascends)
            if "centroid" in stats or "covariance" in stats:
                cen = np.array([tree_sum(p[:, c]) / m for c in range(3)])
                out["centroid"][:, s] = cen
                if "covariance" in stats:
                    d = p - cen
                    for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                        out["covariance"][e, s] = tree_sum(d[:, i] * d[:, j]) / m
            if "value_mean" in stats or "value_variance" in stats:
                mean = tree_sum(w) / m
                out["value_mean"][0, s] = mean
                if "value_variance" in stats:
                    d = w - mean
                    out["value_variance"][0, s] = tree_sum(d * d) / m
    return {s: out[s] for s in stats}, apex, int(counts.sum())


def planes(result, stats):
    """the [planes][S] array pst_segment_statistics writes for these statistics: ascending bit order"""
    return np.concatenate([result[s] for s in STATS if s in stats], axis=0)
