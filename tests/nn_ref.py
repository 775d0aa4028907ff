"""Nearest neighbours between two clouds and the ICP step restated in numpy (the definitions of include/pasture_amd.h, "Nearest neighbours
between two clouds, ICP").

A query q goes through the optional transform first, x' = ((r00*x + r01*y) + r02*z) + t0; its match is the finite target p with the smallest
d2 = (dx*dx + dy*dy) + dz*dz, dx = p.x - q'.x, among those with d2 <= m2 = max_distance * max_distance, equal d2 going to the lower target
index; every operation one rounded f64 operation (numpy evaluates the expressions exactly so).  No match: 0xFFFFFFFF and +inf.

nearest is the definition (all pairs, in chunks); nearest_grid finds the same matches by the clamped-cell ring walk on a numpy grid with a cell
edge of the caller's choosing, and shares no code with the device but the idea.  icp_step returns the sums with math.fsum accuracy and the
rotation by numpy's SVD (Kabsch with the determinant correction)."""
import math

import numpy as np

NONE = 0xFFFFFFFF
_CHUNK = 1 << 22  # pairs tested per numpy expression


def _points(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def apply_transform(points, transform):
    """Rows of `points` through the 3 x 4 (or 12-element) row-major [R | t], with the roundings of the definition; None: the points themselves."""
    q = _points(points)
    if transform is None:
        return q
    t = np.asarray(transform, dtype=np.float64).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((t[a, 0] * q[:, 0] + t[a, 1] * q[:, 1]) + t[a, 2] * q[:, 2]) + t[a, 3] for a in range(3)], axis=1)


def squared_distances(q, p):
    """d2 of rows of q (queries, already transformed) against rows of p (targets): target minus query."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def _m2(max_distance):
    return np.float64(max_distance) * np.float64(max_distance)


def nearest(query, target, max_distance=np.inf, transform=None):
    """(idx uint32, dist float64) of the definition, by brute force."""
    q, p = apply_transform(query, transform), _points(target)
    nq, m2 = len(q), _m2(max_distance)
    idx, best = np.full(nq, NONE, dtype=np.uint32), np.full(nq, np.inf)
    tf = np.flatnonzero(np.isfinite(p).all(axis=1))  # ascending: argmin's first hit is the lowest buffer index
    qf = np.flatnonzero(np.isfinite(q).all(axis=1))
    if tf.size and qf.size:
        pf = p[tf]
        rows = max(1, _CHUNK // len(pf))
        for i0 in range(0, len(qf), rows):
            sel = qf[i0:i0 + rows]
            d2 = squared_distances(q[sel, None, :], pf[None, :, :])
            j = np.argmin(d2, axis=1)
            dmin = d2[np.arange(len(sel)), j]
            ok = dmin <= m2
            idx[sel[ok]] = tf[j[ok]]
            best[sel[ok]] = dmin[ok]
    dist = np.where(idx != NONE, np.sqrt(best), np.inf)
    return idx, dist


def nearest_grid(query, target, edge, max_distance=np.inf, transform=None):
    """The same matches by the ring walk: targets in the cells of a grid of cell edge `edge` over their AABB, the query clamped into the AABB,
    rings of cells at Chebyshev distance 0, 1, 2, ... around the clamped query's cell until best_d2 <= (r * edge * (1 - 2^-20))^2 or the grid is
    exhausted.  One query at a time: for the small clouds of the CPU tests."""
    q, p = apply_transform(query, transform), _points(target)
    nq, m2 = len(q), _m2(max_distance)
    idx, dist = np.full(nq, NONE, dtype=np.uint32), np.full(nq, np.inf)
    tf = np.flatnonzero(np.isfinite(p).all(axis=1))
    if not tf.size:
        return idx, dist
    pf = p[tf]
    lo, hi = pf.min(axis=0), pf.max(axis=0)
    edge = float(edge)
    cells = np.floor((pf - lo) / edge).astype(np.int64)
    dim = cells.max(axis=0) + 1
    stop = edge * (1.0 - 2.0 ** -20)
    for i in range(nq):
        if not np.isfinite(q[i]).all():
            continue
        c = np.floor((np.clip(q[i], lo, hi) - lo) / edge).astype(np.int64)
        ring = np.abs(cells - c).max(axis=1)  # every target's ring around the clamped query's cell
        best, who = m2, NONE
        rmax = int(max(np.max(c), np.max(dim - 1 - c)))
        r = 0
        while True:
            ks = np.flatnonzero(ring == r)
            for k, d in zip(ks, squared_distances(q[i][None, :], pf[ks])):
                if d < best or (d == best and tf[k] < who):
                    best, who = d, tf[k]
            if r >= rmax or best <= (r * stop) * (r * stop):
                break
            r += 1
        if who != NONE:
            idx[i], dist[i] = who, np.sqrt(best)
    return idx, dist


def _fsum_columns(a):
    return np.array([math.fsum(col) for col in np.asarray(a, dtype=np.float64).reshape(len(a), -1).T])


def kabsch(H):
    """The proper rotation R that maximises trace(R H): H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T."""
    U, _, Vt = np.linalg.svd(np.asarray(H, dtype=np.float64).reshape(3, 3))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T


def compose(dR, dt, T_in):
    """(dR | dt) o T_in as a 3 x 4"""
    T_in = np.asarray(T_in, dtype=np.float64).reshape(3, 4)
    return np.column_stack([dR @ T_in[:, :3], dR @ T_in[:, 3] + dt])


def icp_step(query, target, T, max_distance, origin=None, idx=None):
    """One step of the definition with T_in = T.  Returns a dict: m; the sums cq, cp, H, sum_d2 (fsum accuracy); abs = the sum of the absolute
    values of the terms of each of those sums (what the tests' error bound scales with: for cq and cp the terms (q' - o) / m, (p - o) / m);
    dR (Kabsch of H), dt, T_out, rms.  origin: the o of the first pass (default: the finite targets' minimum, which is the index's grid origin)."""
    q, p = apply_transform(query, T), _points(target)
    if idx is None:  # (idx: what nearest returned for these arguments, when the caller has it already)
        idx, _ = nearest(query, target, max_distance, T)
    sel = np.flatnonzero(idx != NONE)
    m = len(sel)
    out = {"m": m, "idx": idx}
    if m == 0:
        return out
    o = p[np.isfinite(p).all(axis=1)].min(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
    qm, pm = q[sel], p[idx[sel]]
    cq, cp = o + _fsum_columns(qm - o) / m, o + _fsum_columns(pm - o) / m
    a, b = qm - cq, pm - cp
    terms = a[:, :, None] * b[:, None, :]
    d2 = squared_distances(qm, pm)
    H, sum_d2 = _fsum_columns(terms).reshape(3, 3), math.fsum(d2)
    dR = kabsch(H)
    dt = cp - dR @ cq
    out.update(cq=cq, cp=cp, H=H, sum_d2=sum_d2, dR=dR, dt=dt, T_out=compose(dR, dt, T), rms=math.sqrt(sum_d2 / m),
               abs={"cq": _fsum_columns(np.abs(qm - o)) / m, "cp": _fsum_columns(np.abs(pm - o)) / m, "H": _fsum_columns(np.abs(terms)).reshape(3, 3),
                    "sum_d2": math.fsum(np.abs(d2))})
    return out
