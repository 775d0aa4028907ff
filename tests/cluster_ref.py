"""Euclidean cluster extraction restated in numpy (the definition of include/pasture_amd.h, "Euclidean cluster extraction").

Finite points i and j are adjacent iff (dx*dx + dy*dy) + dz*dz <= t2 with dx = pj.x - pi.x and t2 = tolerance * tolerance, every operation one
rounded f64 operation (numpy evaluates the expression exactly so); a cluster is a connected component; clusters of min_size .. max_size points
are kept and numbered by descending size, ties by ascending smallest member index; a point in no kept cluster carries 0xFFFFFFFF.

components_brute is the definition (all pairs); components_grid finds the same edges through a cell sort whose cell edge is 2 x tolerance, so it
shares no knife edge with the device grid (cell edge just above the tolerance).  Both return, per point, the smallest index of its component
(-1 for a point that is not finite)."""
import numpy as np

NONE = 0xFFFFFFFF
_CHUNK = 1 << 22  # candidate pairs tested per numpy expression


def adjacent(p, q, t2):
    """The predicate on rows of p and q (q minus p, as the header writes it).  Non-finite coordinates compare false."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
        return (dx * dx + dy * dy) + dz * dz <= t2


def union_find(n, a, b):
    """Components of the graph with edges (a[k], b[k]) on n nodes: parent[v] <= v throughout; every round hooks the larger of two neighbouring
    roots under the smallest neighbouring root it has and then compresses every path, until no edge joins two roots.  Returns the root of every
    node, which is the smallest node of its component."""
    parent = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        if not a.size:
            break
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return parent


def union_find_plain(n, a, b):
    """The textbook sequential form, for the small clouds the vectorised one is checked against."""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for i, j in zip(a, b):
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def _finish(n, finite, a, b):
    comp = union_find(n, a, b)
    comp[~finite] = -1
    return comp


def components_brute(points, tolerance, plain=False):
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    n = len(pts)
    t2 = np.float64(tolerance) * np.float64(tolerance)
    finite = np.isfinite(pts).all(axis=1)
    ea, eb = [], []
    rows = max(1, _CHUNK // max(n, 1))
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        adj = adjacent(pts[i0:i1, None, :], pts[None, :, :], t2) & finite[None, :] & finite[i0:i1, None]
        i, j = np.nonzero(adj)
        keep = j < i + i0
        ea.append(i[keep] + i0)
        eb.append(j[keep])
    a = np.concatenate(ea) if ea else np.zeros(0, dtype=np.int64)
    b = np.concatenate(eb) if eb else np.zeros(0, dtype=np.int64)
    if plain:
        comp = union_find_plain(n, a, b)
        comp[~finite] = -1
        return comp
    return _finish(n, finite, a, b)


def _compact_axis(c):
    """Cell numbers of one axis renumbered without gaps that matter: every c, c - 1 and c + 1 keeps its distance of 1 (no integer lies between
    them), everything else only its order.  Returns (new numbers, how many there are)."""
    u = np.unique(np.concatenate([c - 1, c, c + 1]))
    return np.searchsorted(u, c), len(u)


def components_grid(points, tolerance):
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    n = len(pts)
    t2 = np.float64(tolerance) * np.float64(tolerance)
    finite = np.isfinite(pts).all(axis=1)
    idx = np.flatnonzero(finite)
    if idx.size == 0:
        return np.full(n, -1, dtype=np.int64)
    p = pts[idx]
    cell = np.floor((p - p.min(axis=0)) / (2.0 * float(tolerance))).astype(np.int64)  # adjacent points: at most one cell apart, with a wide margin
    cx, nx = _compact_axis(cell[:, 0])
    cy, ny = _compact_axis(cell[:, 1])
    cz, nz = _compact_axis(cell[:, 2])
    assert nx * ny * nz < 2 ** 62
    key = (cz * ny + cy) * nx + cx
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ukey, start, count = np.unique(skey, return_index=True, return_counts=True)
    ps, pidx = p[order], idx[order]
    ea, eb = [], []
    # the cell itself and the 13 cells of the half stencil that follow it in key order
    offsets = [(0, 0, 0)] + [(dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]
    for dx, dy, dz in offsets:
        target = ukey + (dz * ny + dy) * nx + dx
        at = np.minimum(np.searchsorted(ukey, target), len(ukey) - 1)
        hit = np.flatnonzero(ukey[at] == target)
        sa, ca, sb, cb = start[hit], count[hit], start[at[hit]], count[at[hit]]
        pairs = ca * cb
        ends = np.cumsum(pairs)
        c0 = 0
        while c0 < len(hit):  # cell pairs in batches of about _CHUNK point pairs
            c1 = int(np.searchsorted(ends, (ends[c0 - 1] if c0 else 0) + _CHUNK, side="left")) + 1
            c1 = min(max(c1, c0 + 1), len(hit))
            m = pairs[c0:c1]
            t = np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)
            i = np.repeat(sa[c0:c1], m) + t // np.repeat(cb[c0:c1], m)
            j = np.repeat(sb[c0:c1], m) + t % np.repeat(cb[c0:c1], m)
            if (dx, dy, dz) == (0, 0, 0):
                low = j < i
                i, j = i[low], j[low]
            adj = adjacent(ps[i], ps[j], t2)
            ea.append(pidx[i[adj]])
            eb.append(pidx[j[adj]])
            c0 = c1
    return _finish(n, finite, np.concatenate(ea), np.concatenate(eb))


def label_components(comp, min_size=1, max_size=2 ** 64 - 1):
    """(labels uint32, sizes uint64) from the per-point component (its smallest member's index, -1 for none)."""
    comp = np.asarray(comp, dtype=np.int64)
    n = len(comp)
    labels = np.full(n, NONE, dtype=np.uint32)
    size = np.bincount(comp[comp >= 0], minlength=n) if n else np.zeros(0, dtype=np.int64)
    roots = np.flatnonzero((size >= min(min_size, n + 1)) & (size >= 1) & (size <= min(max_size, n)))
    roots = roots[np.lexsort((roots, -size[roots]))]  # descending size, then ascending smallest member (= the root)
    number = np.full(n, NONE, dtype=np.uint32)
    number[roots] = np.arange(len(roots), dtype=np.uint32)
    member = comp >= 0
    labels[member] = number[comp[member]]
    return labels, size[roots].astype(np.uint64)


def label(points, tolerance, min_size=1, max_size=2 ** 64 - 1, grid=None):
    """(labels, sizes) of the definition; brute force up to 4096 points, the cell sort above that (grid=True / False forces one)."""
    n = len(np.asarray(points).reshape(-1, 3))
    use_grid = n > 4096 if grid is None else grid
    comp = components_grid(points, tolerance) if use_grid else components_brute(points, tolerance)
    return label_components(comp, min_size, max_size)
