"""The numpy restatement of the point-in-polygon definition (include/pasture_amd.h, "Polygon crop and overlay") and of the y-band directory
(pasture_amd/csrc/polygon_index.hpp).  It evaluates EVERY edge of every polygon for every point: no index, no box, no shortcut.  Every
operation is one numpy f64 operation, rounded once, in the order the header writes them."""
import numpy as np

NO_POLYGON = 0xFFFFFFFF
MAX_AUTO_BANDS = 1 << 16
AUTO_ENTRIES_PER_BAND = 8
MAX_DIRECTORY_ENTRIES = 1 << 27


def rings_of(polygons):
    """[(polygon index, (m, 2) float64 ring)]: a polygon is one (m, 2) array or a list of them"""
    out = []
    for p, polygon in enumerate(polygons):
        try:
            a = np.asarray(polygon, dtype=np.float64)
        except ValueError:
            a = None
        for ring in ([a] if a is not None and a.ndim == 2 else [np.asarray(r, dtype=np.float64) for r in polygon]):
            assert ring.ndim == 2 and ring.shape[1] == 2 and len(ring) >= 3 and np.isfinite(ring).all()
            out.append((p, ring))
    return out


def entries_of(polygons):
    """(entries (E, 4) float64 {lo.x, lo.y, hi.x, hi.y}, polygon (E,) uint32) in input order; horizontal edges are dropped"""
    ent, pol = [], []
    for p, ring in rings_of(polygons):
        m = len(ring)
        for i in range(m):
            a, b = ring[i], ring[(i + 1) % m]
            if a[1] == b[1]:
                continue
            lo, hi = (a, b) if a[1] < b[1] else (b, a)
            ent.append((lo[0], lo[1], hi[0], hi[1]))
            pol.append(p)
    return np.asarray(ent, dtype=np.float64).reshape(-1, 4), np.asarray(pol, dtype=np.uint32)


def crossings(x, y, entry):
    """bool per point: does it cross this entry?  (x, y finite is the caller's test)"""
    lox, loy, hix, hiy = (np.float64(v) for v in entry)
    with np.errstate(all="ignore"):
        d = (hix - lox) * (y - loy) - (x - lox) * (hiy - loy)
    return (loy <= y) & (y < hiy) & (d > 0.0) & np.isfinite(d)


def contains(pts, polygon):
    """bool per point: in this ONE polygon (an (m, 2) ring or a list of rings)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    x, y = pts[:, 0], pts[:, 1]
    ent, _ = entries_of([polygon])
    odd = np.zeros(len(pts), dtype=bool)
    for e in ent:
        odd ^= crossings(x, y, e)
    return odd & np.isfinite(x) & np.isfinite(y)


def point_ids(pts, polygons):
    """uint32 per point: the smallest index of a polygon that contains it, NO_POLYGON without one"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    ids = np.full(len(pts), NO_POLYGON, dtype=np.uint32)
    for p in range(len(polygons) - 1, -1, -1):  # descending: the smallest index is written last
        ids[contains(pts, polygons[p])] = p
    return ids


def mask_of(ids, outside=False):
    """(mask uint8, count)"""
    mask = ((ids != NO_POLYGON) != bool(outside)).astype(np.uint8)
    return mask, int(mask.sum())


# ---- the band directory -----------------------------------------------------------------------------------------------------------------------

def band_of(y, ymin, scale, bands):
    with np.errstate(all="ignore"):
        t = (np.asarray(y, dtype=np.float64) - np.float64(ymin)) * np.float64(scale)
        return np.where(t >= 1.0, np.minimum(np.floor(t), bands - 1), 0).astype(np.int64)  # (a NaN t fails t >= 1: band 0)


def directory(polygons, bands=0):
    """{"bands", "ymin", "scale", "box", "entries", "polygon", "lists": per band the entry indices in input order}"""
    ent, pol = entries_of(polygons)
    v = np.concatenate([r for _, r in rings_of(polygons)])
    box = (v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max())
    ymin, ymax = box[1], box[3]

    def spans(count):
        with np.errstate(all="ignore"):
            scale = np.float64(count) / (np.float64(ymax) - np.float64(ymin))
        return scale, band_of(ent[:, 1], ymin, scale, count), band_of(ent[:, 3], ymin, scale, count)
    if bands:
        scale, first, last = spans(bands)
    else:
        bands = min(max((len(ent) + AUTO_ENTRIES_PER_BAND - 1) // AUTO_ENTRIES_PER_BAND, 1), MAX_AUTO_BANDS)
        while True:
            scale, first, last = spans(bands)
            if int((last - first + 1).sum()) <= MAX_DIRECTORY_ENTRIES:
                break
            bands //= 2
    assert (first <= last).all()
    lists = [[] for _ in range(bands)]
    for e in range(len(ent)):
        for b in range(first[e], last[e] + 1):
            lists[b].append(e)
    return {"bands": bands, "ymin": ymin, "scale": float(scale), "box": box, "entries": ent, "polygon": pol, "lists": lists}


# ---- shapes the tests share --------------------------------------------------------------------------------------------------------------------

def rectangle(x0, y0, x1, y1, reverse=False):
    r = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)
    return r[::-1].copy() if reverse else r


def grid_rectangles(xs, ys):
    """one rectangle per cell of the grid lines xs x ys, row-major with x fastest; every other one runs the other way round"""
    out = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            out.append(rectangle(xs[i], ys[j], xs[i + 1], ys[j + 1], reverse=(i + j) % 2 == 1))
    return out


def grid_cell_ids(pts, xs, ys):
    """what comparisons against the grid lines give: the cell with xs[i] <= x < xs[i + 1] and ys[j] <= y < ys[j + 1]"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    i = np.searchsorted(xs, pts[:, 0], side="right") - 1
    j = np.searchsorted(ys, pts[:, 1], side="right") - 1
    inside = (i >= 0) & (i < len(xs) - 1) & (j >= 0) & (j < len(ys) - 1) & np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1])
    return np.where(inside, j * (len(xs) - 1) + i, NO_POLYGON).astype(np.uint32)


def star(n_vertices, centre=(0.0, 0.0), r_outer=1.0, r_inner=0.45, phase=0.1):
    a = phase + 2.0 * np.pi * np.arange(n_vertices) / n_vertices
    r = np.where(np.arange(n_vertices) % 2 == 0, r_outer, r_inner)
    return np.column_stack([centre[0] + r * np.cos(a), centre[1] + r * np.sin(a)])


def fan(n_triangles=40, centre=(7.0e5, 7.0e5), radius=100.0):
    """(triangles, outline): a fan of triangles around the centre, every other one running the other way round, and the rim polygon"""
    a = 0.05 + 2.0 * np.pi * np.arange(n_triangles) / n_triangles
    rim = np.column_stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)])
    c = np.asarray(centre, dtype=np.float64)
    tris = []
    for k in range(n_triangles):
        t = np.array([c, rim[k], rim[(k + 1) % n_triangles]])
        tris.append(t[::-1].copy() if k % 2 else t)
    return tris, rim
