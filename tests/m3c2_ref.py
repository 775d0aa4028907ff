"""M3C2 change detection restated in numpy (the definitions of include/pasture_amd.h, "M3C2 change detection").

Every point of a cloud is tested against every core point, with no grid, in chunks; the expressions are the header's, literally, and numpy
evaluates each operation as one rounded f64 operation.  Per member the restatement takes t and t*t -- the very bits the device adds -- and sums
them with math.fsum; it also returns sum |t| and sum t*t, from which the tests bound what ANY order of summation may differ from the fsum value.
The normal of the nearest reference point comes from tests/nn_ref.py."""
import math

import numpy as np

import nn_ref

ORIENT_UP = 1
_CHUNK = 1 << 22  # pairs tested per numpy expression


def _points(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def nearest_normals(core, reference_points, reference_normals):
    """(normals (n, 3), found (n,)): the normal stored for the nearest reference point of every core point (nn_ref.nearest: unbounded, no
    transform, ties to the lower buffer index); found is False where there is none."""
    core, normals = _points(core), _points(reference_normals)
    idx, _ = nn_ref.nearest(core, reference_points)
    found = idx != nn_ref.NONE
    out = np.zeros((len(core), 3))
    out[found] = normals[idx[found]]
    return out, found


def unit_normals(core, normals, flags=0, found=None):
    """(u (n, 3), valid (n,)): u = n / sqrt((nx*nx + ny*ny) + nz*nz), flipped upwards with ORIENT_UP; three NaNs for an invalid core point."""
    c, nrm = _points(core), _points(normals)
    with np.errstate(all="ignore"):
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        s = np.sqrt(nn)
        u = np.stack([nrm[:, 0] / s, nrm[:, 1] / s, nrm[:, 2] / s], axis=1)
    valid = np.isfinite(c).all(axis=1) & np.isfinite(nrm).all(axis=1) & (nn != 0.0) & np.isfinite(nn)
    if found is not None:
        valid &= found
    if flags & ORIENT_UP:
        down = (u[:, 2] < 0.0) | ((u[:, 2] == 0.0) & ((u[:, 1] < 0.0) | ((u[:, 1] == 0.0) & (u[:, 0] < 0.0))))
        u[down] = -u[down]
    u[~valid] = np.nan
    return u, valid


def member_terms(c, u, cloud, radius, max_depth):
    """t of the members of ONE core point's cylinder among the finite rows of `cloud`, in cloud order"""
    with np.errstate(all="ignore"):
        dx, dy, dz = cloud[:, 0] - c[0], cloud[:, 1] - c[1], cloud[:, 2] - c[2]
        t = (dx * u[0] + dy * u[1]) + dz * u[2]
        wx, wy, wz = dx - t * u[0], dy - t * u[1], dz - t * u[2]
        r2 = (wx * wx + wy * wy) + wz * wz
        inside = (np.abs(t) <= max_depth) & (r2 <= np.float64(radius) * np.float64(radius))
    return t[inside]


def cylinders(core, u, valid, cloud, radius, max_depth):
    """Per core point over one cloud: counts (n,) uint32, sums (n, 2) = fsum t, fsum t*t, and abs (n, 2) = sum |t|, sum t*t."""
    core, cloud = _points(core), _points(cloud)
    cloud = cloud[np.isfinite(cloud).all(axis=1)]
    n = len(core)
    counts, sums, absum = np.zeros(n, dtype=np.uint32), np.zeros((n, 2)), np.zeros((n, 2))
    if len(cloud) == 0:
        return counts, sums, absum
    R2, L = np.float64(radius) * np.float64(radius), np.float64(max_depth)
    rows = max(1, _CHUNK // len(cloud))
    good = np.flatnonzero(valid)
    for i0 in range(0, len(good), rows):
        sel = good[i0:i0 + rows]
        c, v = core[sel, None, :], u[sel, None, :]
        with np.errstate(all="ignore"):
            dx, dy, dz = cloud[None, :, 0] - c[..., 0], cloud[None, :, 1] - c[..., 1], cloud[None, :, 2] - c[..., 2]
            t = (dx * v[..., 0] + dy * v[..., 1]) + dz * v[..., 2]
            wx, wy, wz = dx - t * v[..., 0], dy - t * v[..., 1], dz - t * v[..., 2]
            r2 = (wx * wx + wy * wy) + wz * wz
            inside = (np.abs(t) <= L) & (r2 <= R2)
        for k, i in enumerate(sel):
            tm = t[k, inside[k]]
            if tm.size:
                tt = tm * tm
                counts[i] = tm.size
                sums[i] = math.fsum(tm), math.fsum(tt)
                absum[i] = math.fsum(np.abs(tm)), math.fsum(tt)
    return counts, sums, absum


def finish(counts, sums, valid, min_points, registration_error):
    """(distance, lod, significant) from counts (n, 2) and sums (n, 4) = St_1, Stt_1, St_2, Stt_2, in the header's order of operations."""
    counts, sums = np.asarray(counts), np.asarray(sums, dtype=np.float64)
    n1, n2 = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
    ok = np.asarray(valid, dtype=bool) & (n1 >= min_points) & (n2 >= min_points)
    with np.errstate(all="ignore"):
        m1, m2 = n1.astype(np.float64), n2.astype(np.float64)
        mean1, mean2 = sums[:, 0] / m1, sums[:, 2] / m2
        distance = mean2 - mean1
        q1 = sums[:, 1] - (sums[:, 0] * sums[:, 0]) / m1
        q2 = sums[:, 3] - (sums[:, 2] * sums[:, 2]) / m2
        var1 = np.where(q1 > 0.0, q1, 0.0) / (n1 - 1).astype(np.float64)
        var2 = np.where(q2 > 0.0, q2, 0.0) / (n2 - 1).astype(np.float64)
        lod = 1.96 * (np.sqrt(var1 / m1 + var2 / m2) + np.float64(registration_error))
        lod[(n1 < 2) | (n2 < 2)] = np.nan
        distance[~ok] = np.nan
        lod[~ok] = np.nan
        significant = np.abs(distance) > lod
    return distance, lod, significant


def m3c2(core, reference, compared, radius, max_depth, normals=None, reference_normals=None, min_points=4, registration_error=0.0, flags=0):
    """The whole definition: a dict of u, valid, counts (n, 2), sums (n, 4), abs (n, 4), distance, lod, significant."""
    core = _points(core)
    if normals is None:
        normals, found = nearest_normals(core, reference, reference_normals)
    else:
        found = None
    u, valid = unit_normals(core, normals, flags, found)
    c1, s1, a1 = cylinders(core, u, valid, reference, radius, max_depth)
    c2, s2, a2 = cylinders(core, u, valid, compared, radius, max_depth)
    counts = np.stack([c1, c2], axis=1)
    sums, absum = np.concatenate([s1, s2], axis=1), np.concatenate([a1, a2], axis=1)
    distance, lod, significant = finish(counts, sums, valid, min_points, registration_error)
    return {"u": u, "valid": valid, "counts": counts, "sums": sums, "abs": absum, "distance": distance, "lod": lod, "significant": significant}
