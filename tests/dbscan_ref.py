"""DBSCAN restated in numpy (the definition of include/pasture_amd.h, "DBSCAN").

Finite points i and j are neighbours iff (dx*dx + dy*dy) + dz*dz <= e2 with dx = pj.x - pi.x and e2 = eps * eps, every operation one rounded f64
operation (cluster_ref.adjacent, which numpy evaluates exactly so); a finite point is its own neighbour.  A finite point with at least
min_points neighbours, itself included, is core.  A cluster is a connected component of the neighbour graph restricted to the core points.  A
finite point that is not core joins the cluster of the core neighbour of smallest (d2, index) and unites nothing; without a core neighbour it is
noise.  Clusters are numbered by descending size (core + border), ties by ascending smallest member index; noise and non-finite points carry
0xFFFFFFFF.

pairs_brute is the definition (all pairs); pairs_grid finds the same pairs through a cell sort whose cell edge is 1.25 x eps, so it shares no
knife edge with the device grid (cell edge just above eps).  Both return every ordered neighbour pair (i, j, d2), i == j included."""
import numpy as np

import cluster_ref as C

NONE = C.NONE
_CHUNK = 1 << 22  # candidate pairs tested per numpy expression


def _d2(p, q):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def _points(points):
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    return pts, np.isfinite(pts).all(axis=1)


def pairs_brute(points, eps):
    pts, finite = _points(points)
    n = len(pts)
    e2 = np.float64(eps) * np.float64(eps)
    ii, jj, dd = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    rows = max(1, _CHUNK // max(n, 1))
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        p, q = pts[i0:i1, None, :], pts[None, :, :]
        adj = C.adjacent(p, q, e2) & finite[None, :] & finite[i0:i1, None]
        i, j = np.nonzero(adj)
        ii.append(i + i0)
        jj.append(j)
        dd.append(_d2(pts[i + i0], pts[j]))
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)


def pairs_grid(points, eps):
    pts, finite = _points(points)
    e2 = np.float64(eps) * np.float64(eps)
    idx = np.flatnonzero(finite)
    if idx.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    p = pts[idx]
    cell = np.floor((p - p.min(axis=0)) / (1.25 * float(eps))).astype(np.int64)  # neighbours: at most one cell apart, with a wide margin
    cx, nx = C._compact_axis(cell[:, 0])
    cy, ny = C._compact_axis(cell[:, 1])
    cz, nz = C._compact_axis(cell[:, 2])
    assert nx * ny * nz < 2 ** 62
    key = (cz * ny + cy) * nx + cx
    order = np.argsort(key, kind="stable")
    ukey, start, count = np.unique(key[order], return_index=True, return_counts=True)
    ps, pidx = p[order], idx[order]
    ii, jj, dd = [idx], [idx], [np.zeros(len(idx))]  # every finite point and itself: d2 = 0 <= e2
    # the cell itself (pairs j < i) and the 13 cells of the half stencil that follow it in key order; every pair found goes in both ways
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
            adj = C.adjacent(ps[i], ps[j], e2)
            i, j = i[adj], j[adj]
            ii += [pidx[i], pidx[j]]
            jj += [pidx[j], pidx[i]]
            dd += [_d2(ps[i], ps[j]), _d2(ps[j], ps[i])]
            c0 = c1
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)


def from_pairs(n, finite, i, j, d2, min_points):
    """(labels uint32, sizes uint64, core bool) from every ordered neighbour pair."""
    degree = np.bincount(i, minlength=n) if n else np.zeros(0, dtype=np.int64)
    core = finite & (degree >= min(int(min_points), n + 1))
    # clusters of the core points: the smallest core index of the component names it for now
    both = core[i] & core[j] & (j < i)
    comp = C.union_find(n, i[both], j[both])
    comp[~core] = -1
    # border points: the core neighbour of smallest (d2, index)
    rim = ~core[i] & core[j]
    bi, bj, bd = i[rim], j[rim], d2[rim]
    by = np.lexsort((bj, bd, bi))  # by point, then distance, then the neighbour's index
    bi, bj = bi[by], bj[by]
    first = np.flatnonzero(np.concatenate([[True], bi[1:] != bi[:-1]])) if len(bi) else np.zeros(0, dtype=np.int64)
    comp[bi[first]] = comp[bj[first]]
    # numbering: descending size, then ascending smallest member
    member = np.flatnonzero(comp >= 0)
    labels = np.full(n, NONE, dtype=np.uint32)
    if member.size == 0:
        return labels, np.zeros(0, dtype=np.uint64), core
    size = np.bincount(comp[member], minlength=n)
    smallest = np.full(n, n, dtype=np.int64)
    np.minimum.at(smallest, comp[member], member)
    names = np.flatnonzero(size > 0)
    names = names[np.lexsort((smallest[names], -size[names]))]
    number = np.full(n, NONE, dtype=np.uint32)
    number[names] = np.arange(len(names), dtype=np.uint32)
    labels[member] = number[comp[member]]
    return labels, size[names].astype(np.uint64), core


def dbscan(points, eps, min_points, grid=None):
    """(labels, sizes, core) of the definition; brute force up to 4096 points, the cell sort above that (grid=True / False forces one)."""
    pts, finite = _points(points)
    use_grid = len(pts) > 4096 if grid is None else grid
    i, j, d2 = pairs_grid(pts, eps) if use_grid else pairs_brute(pts, eps)
    return from_pairs(len(pts), finite, i, j, d2, min_points)
