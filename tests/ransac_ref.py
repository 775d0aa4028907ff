"""Restatement of the RANSAC plane / line contract (pasture-algorithms/src/segmentation.rs) in numpy float64 and Python integers.

Vectorised over points, one hypothesis at a time, every operation written out in the contract's order: numpy's `*`, `+`, `-`, `/` and `sqrt` on
float64 are the correctly rounded IEEE operations (no np.dot, np.cross or np.linalg.norm, whose summation order is theirs to choose).
  plane from (i1, i2, i3): v1 = p2 - p1, v2 = p3 - p1, n = v1 x v2, d = -((n.x*p1.x + n.y*p1.y) + n.z*p1.z)
  plane inlier: |((a*x + b*y) + c*z) + d| / sqrt((a*a + b*b) + c*c) < thr
  line inlier:  sqrt((cx*cx + cy*cy) + cz*cz) / sqrt((dx*dx + dy*dy) + dz*dz) < thr, c = (second - first) x (first - p), d = second - first
  cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
  winner: the highest ranking, the LAST such iteration on ties (Iterator::max_by)
"""
import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample_indices(seed, n, iterations, per):
    """One counter per call, from 0, one step per draw (redraws included); draw = (splitmix64(seed ^ c) * n) >> 64."""
    c = 0

    def draw():
        nonlocal c
        u = splitmix64((seed ^ c) & M64)
        c += 1
        return (u * n) >> 64

    out = []
    for _ in range(iterations):
        r1 = draw()
        r2 = draw()
        while r1 == r2:
            r2 = draw()
        row = [r1, r2]
        if per == 3:
            r3 = draw()
            while r2 == r3 or r1 == r3:
                r3 = draw()
            row.append(r3)
        out.append(row)
    return np.array(out, dtype=np.uint64).reshape(iterations, per)


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def plane_from(p1, p2, p3):
    with np.errstate(all="ignore"):
        p1, p2, p3 = (np.asarray(p, dtype=np.float64) for p in (p1, p2, p3))
        n = _cross(p2 - p1, p3 - p1)
        d = -((n[0] * p1[0] + n[1] * p1[1]) + n[2] * p1[2])
        return np.array([n[0], n[1], n[2], d], dtype=np.float64)


def plane_inlier_mask(pts, plane, thr):
    with np.errstate(all="ignore"):
        a, b, c, d = (np.float64(v) for v in plane)
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        num = np.abs(((a * x + b * y) + c * z) + d)
        e = np.sqrt((a * a + b * b) + c * c)
        return (num / e) < np.float64(thr)


def line_inlier_mask(pts, line, thr):
    with np.errstate(all="ignore"):
        f = np.asarray(line[0:3], dtype=np.float64)
        s = np.asarray(line[3:6], dtype=np.float64)
        dv = s - f
        w = (f[0] - pts[:, 0], f[1] - pts[:, 1], f[2] - pts[:, 2])
        cx, cy, cz = _cross(dv, w)
        num = np.sqrt((cx * cx + cy * cy) + cz * cz)
        den = np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
        return (num / den) < np.float64(thr)


def model_from(pts, sample, line):
    if line:
        return np.concatenate([pts[int(sample[0])], pts[int(sample[1])]]).astype(np.float64)
    return plane_from(pts[int(sample[0])], pts[int(sample[1])], pts[int(sample[2])])


def inlier_mask(pts, model, thr, line):
    return line_inlier_mask(pts, model, thr) if line else plane_inlier_mask(pts, model, thr)


def ransac(pts, thr, samples, line):
    """(winning model, its ranking, winning iteration, rankings of all hypotheses, inlier indices of the winner)."""
    pts = np.asarray(pts, dtype=np.float64)
    rankings = np.zeros(len(samples), dtype=np.uint64)
    models = []
    for it, s in enumerate(samples):
        m = model_from(pts, s, line)
        models.append(m)
        rankings[it] = np.count_nonzero(inlier_mask(pts, m, thr, line))
    best = 0
    for it in range(len(samples)):  # max_by keeps the last of equal maxima
        if rankings[it] >= rankings[best]:
            best = it
    idx = np.flatnonzero(inlier_mask(pts, models[best], thr, line)).astype(np.uint64)
    return models[best], int(rankings[best]), best, rankings, idx


def reference_test_cloud():
    """segmentation.rs:388-410 by formula: p = 2 .. 2001 -> (p, p*p, 1); every fifth on the z axis (0, 0, p*p); (every fiftieth: z = p*p, already so)."""
    p = np.arange(2, 2002, dtype=np.float64)
    pts = np.stack([p, p * p, np.ones_like(p)], axis=1)
    on_axis = (np.arange(2, 2002) % 5) == 0
    pts[on_axis] = np.stack([np.zeros_like(p), np.zeros_like(p), p * p], axis=1)[on_axis]
    return pts


def doc_plane_cloud():
    """:160-167: (0, i, i*i) for i < 200, then the outlier (9, 0, 0)."""
    i = np.arange(200, dtype=np.float64)
    return np.concatenate([np.stack([np.zeros_like(i), i, i * i], axis=1), [[9.0, 0.0, 0.0]]])


def doc_line_cloud():
    """:276-282: (0, 0, i) for i < 200, then the outlier (9, 0, 0)."""
    i = np.arange(200, dtype=np.float64)
    return np.concatenate([np.stack([np.zeros_like(i), np.zeros_like(i), i], axis=1), [[9.0, 0.0, 0.0]]])
