"""Fixed-radius neighbour search restated in numpy (the definitions of include/pasture_amd.h, "Fixed-radius neighbour search").

A query q goes through the optional transform first, x' = ((r00*x + r01*y) + r02*z) + t0 (nn_ref.apply_transform); a finite target p is a
neighbour iff d2 = (dx*dx + dy*dy) + dz*dz <= r2, dx = p.x - q'.x, r2 = radius * radius, every operation one rounded f64 operation (numpy
evaluates the expressions exactly so); the bound is inclusive.  A query that is not finite after the transform has no neighbours.  The list
of a query is ordered by ascending (d2, target buffer index); distances are sqrt(d2).  The result is (offsets uint64 (n + 1,), indices uint32,
distances float64).

search is the definition (all pairs, in chunks); search_grid finds the same lists from the buckets of a numpy grid with a cell edge of the
caller's choosing -- whole cells within ceil(radius / edge) of the query's cell, every candidate tested by the same predicate -- and
shares no code with the device."""
import numpy as np

from nn_ref import _points, apply_transform, squared_distances

_CHUNK = 1 << 22  # pairs tested per numpy expression


def _r2(radius):
    return np.float64(radius) * np.float64(radius)


def _csr(n, rows, idx, d2):
    """rows (query of every hit), idx, d2 -> (offsets, indices, distances) with every list ordered by (d2, idx)"""
    order = np.lexsort((idx, d2, rows))
    rows, idx, d2 = rows[order], idx[order], d2[order]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=n)).astype(np.uint64)
    return offsets, idx.astype(np.uint32), np.sqrt(d2)


def search(query, target, radius, transform=None):
    """(offsets, indices, distances) of the definition, by brute force."""
    q, p = apply_transform(query, transform), _points(target)
    r2 = _r2(radius)
    tf = np.flatnonzero(np.isfinite(p).all(axis=1))
    qf = np.flatnonzero(np.isfinite(q).all(axis=1))
    rows, idx, d2s = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    if tf.size and qf.size:
        pf = p[tf]
        step = max(1, _CHUNK // len(pf))
        for i0 in range(0, len(qf), step):
            sel = qf[i0:i0 + step]
            d2 = squared_distances(q[sel, None, :], pf[None, :, :])
            a, b = np.nonzero(d2 <= r2)
            rows.append(sel[a])
            idx.append(tf[b])
            d2s.append(d2[a, b])
    return _csr(len(q), np.concatenate(rows), np.concatenate(idx), np.concatenate(d2s))


def counts(query, target, radius, transform=None):
    return np.diff(search(query, target, radius, transform)[0]).astype(np.uint32)


def search_grid(query, target, radius, edge=None, transform=None):
    """The same lists from a bucketed grid of cell edge `edge` (default: just above the radius) over the finite targets: per offset of the cube of
    cells around a query's cell, the queries are joined with the targets of that cell through the sorted cell keys."""
    q, p = apply_transform(query, transform), _points(target)
    r2 = _r2(radius)
    n = len(q)
    tf = np.flatnonzero(np.isfinite(p).all(axis=1))
    qf = np.flatnonzero(np.isfinite(q).all(axis=1))
    rows, idx, d2s = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    if tf.size and qf.size:
        edge = float(radius) * (1.0 + 2.0 ** -16) if edge is None else float(edge)
        pf, qq = p[tf], q[qf]
        lo = pf.min(axis=0)
        tc = np.floor((pf - lo) / edge).astype(np.int64)
        dim = tc.max(axis=0) + 1
        # a neighbour is at most rho = radius / edge cells away per axis (up to roundings far below 2^-20): its cell number differs by at
        # most ceil(rho); the default edge, just above the radius, makes that one cell
        reach = int(np.ceil(float(radius) / edge + 2.0 ** -20))
        # a query farther than reach cells outside the grid cannot have a neighbour; clip the others' cells into a padded grid
        qc = np.floor(np.clip((qq - lo) / edge, -reach - 1.0, (dim + reach + 1).astype(np.float64))).astype(np.int64)
        stride = np.array([1, dim[0], dim[0] * dim[1]], dtype=np.int64)
        tkey = tc @ stride
        torder = np.argsort(tkey, kind="stable")
        tsorted = tkey[torder]
        for oz in range(-reach, reach + 1):
            for oy in range(-reach, reach + 1):
                for ox in range(-reach, reach + 1):
                    c = qc + np.array([ox, oy, oz])
                    ok = np.flatnonzero(((c >= 0) & (c < dim)).all(axis=1))
                    if not ok.size:
                        continue
                    key = c[ok] @ stride
                    first, last = np.searchsorted(tsorted, key, "left"), np.searchsorted(tsorted, key, "right")
                    m = last - first
                    if not m.sum():
                        continue
                    qi = np.repeat(ok, m)
                    ti = torder[np.repeat(first, m) + (np.arange(m.sum()) - np.repeat(np.cumsum(m) - m, m))]
                    d2 = squared_distances(qq[qi], pf[ti])
                    hit = d2 <= r2
                    rows.append(qf[qi[hit]])
                    idx.append(tf[ti[hit]])
                    d2s.append(d2[hit])
    return _csr(n, np.concatenate(rows), np.concatenate(idx), np.concatenate(d2s))
