"""A numpy restatement of pst_rasterize and pst_grid_fill_device, written from the text of include/pasture_amd.h ("Rasterisation").

Every sum is a plain Python loop over numpy float64 scalars in the order the header gives: np.sum adds pairwise, which is not the
definition.  float64 arithmetic in numpy is IEEE, one rounding per operation, like the kernels' (compiled without contraction)."""
import numpy as np

CHUNK = 256  # PST_RASTER_CHUNK: part of the definition
STATS = ("count", "min", "max", "mean", "variance")  # ascending bit order
NAN_BITS = np.uint64(0x7FF8000000000000)
NAN = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]


def bits(a):
    """the u64 view results are compared through: NaNs as bits, -0.0 apart from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ordered(v):
    """the order-preserving key of a double: -0.0 below +0.0"""
    u = int(np.array([v], dtype=np.float64).view(np.uint64)[0])
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | 0x8000000000000000


def plain_sum(values):
    s = np.float64(values[0])
    for v in values[1:]:
        s = s + np.float64(v)
    return s


def chunked_sum(values):
    """chunk j = values[256 j : 256 (j + 1)], P_j its left-to-right sum from its first element; S = P_0 + P_1 + ... left to right"""
    partials = [plain_sum(values[b:b + CHUNK]) for b in range(0, len(values), CHUNK)]
    return plain_sum(partials)


def auto_grid(pts, cell):
    """pst_pmf_grid: over the points with three finite components; (x0, y0, cols, rows), zeros without one"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    fin = np.isfinite(pts).all(axis=1)
    if not fin.any():
        return 0.0, 0.0, 0, 0
    x0, y0 = pts[fin, 0].min(), pts[fin, 1].min()
    cols = int((pts[fin, 0].max() - x0) / np.float64(cell)) + 1
    rows = int((pts[fin, 1].max() - y0) / np.float64(cell)) + 1
    return float(x0), float(y0), cols, rows


def rasterize(pts, cell, stats=STATS, values=None, mask=None, origin=None, dim=None):
    """-> ({name: (rows, cols) float64}, n_members, (x0, y0, cols, rows))"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cell = np.float64(cell)
    if origin is None:
        x0, y0, cols, rows = auto_grid(pts, cell)
    else:
        (x0, y0), (cols, rows) = origin, dim
    x0, y0 = np.float64(x0), np.float64(y0)
    v = pts[:, 2] if values is None else np.asarray(values, dtype=np.float64)
    members = [[] for _ in range(cols * rows)]
    with np.errstate(all="ignore"):
        for i in range(len(pts)):
            x, y = pts[i, 0], pts[i, 1]
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(v[i])):
                continue
            if mask is not None and mask[i] == 0:
                continue
            qx, qy = (x - x0) / cell, (y - y0) / cell
            if not (qx >= 0.0 and qx < float(cols) and qy >= 0.0 and qy < float(rows)):
                continue
            members[int(qy) * cols + int(qx)].append(v[i])  # ascending buffer index
        out = {s: np.full(cols * rows, NAN, dtype=np.float64) for s in STATS}
        out["count"][:] = 0.0
        for c, vs in enumerate(members):
            m = len(vs)
            if m == 0:
                continue
            out["count"][c] = float(m)
            out["min"][c] = min(vs, key=ordered)
            out["max"][c] = max(vs, key=ordered)
            mean = chunked_sum(vs) / np.float64(m)
            out["mean"][c] = mean
            squares = []
            for t in vs:
                d = np.float64(t) - mean
                squares.append(d * d)
            out["variance"][c] = chunked_sum(squares) / np.float64(m)
    n_members = sum(len(vs) for vs in members)
    return {s: out[s].reshape(rows, cols) for s in stats}, n_members, (float(x0), float(y0), cols, rows)


def fill(raster, h):
    """pst_grid_fill_device: an entry that is not finite becomes the inverse-squared-distance weighted mean of the finite entries of the
    square of h cells around it, visited in row-major order; the canonical NaN without one.  h == 0: a copy."""
    a = np.asarray(raster, dtype=np.float64)
    rows, cols = a.shape
    out = a.copy()
    if h == 0:
        return out
    # every cell at once, one offset after the other: each cell sees its neighbours in row-major order (dr ascending, then dc ascending)
    padded = np.full((rows + 2 * h, cols + 2 * h), NAN, dtype=np.float64)  # outside the raster: never visited
    padded[h:h + rows, h:h + cols] = a
    num, den = np.zeros_like(a), np.zeros_like(a)
    any_visited = np.zeros(a.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for dr in range(-h, h + 1):
            for dc in range(-h, h + 1):
                if dr == 0 and dc == 0:
                    continue  # the cell itself: finite entries are copied, empty ones are not visited
                v = padded[h + dr:h + dr + rows, h + dc:h + dc + cols]
                visit = np.isfinite(v)
                w = np.float64(1.0) / np.float64(dr * dr + dc * dc)
                first, later = visit & ~any_visited, visit & any_visited
                num = np.where(first, w * v, np.where(later, num + w * v, num))
                den = np.where(first, w, np.where(later, den + w, den))
                any_visited |= visit
        filled = np.where(any_visited, num / den, NAN)
    empty = ~np.isfinite(a)
    out[empty] = filled[empty]
    return out


def wide_values(n, seed):
    """n values spanning 30 decades with mixed signs: their sum depends on the order of the additions in its low bits"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15.0, 15.0, n) * rng.uniform(1.0, 2.0, n)
