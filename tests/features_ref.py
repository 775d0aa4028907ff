"""numpy restatement of pst_geometric_features_from_knn_device (include/pasture_amd.h, "Geometric features").

Vectorised over the queries; every arithmetic step is one numpy operation on float64 arrays, that is one rounded IEEE operation per element,
in the order the definition gives.  Where the definition branches per neighbourhood the restatement computes both sides and selects
(np.where), which changes no selected value.  cbrt and log are the C library's (documented within 1 ulp), called per element.

features(pts, knn, max_distance) returns a dict: the thirteen planes by name, "normals" (e3) and "directions" (e1) oriented upwards, "e2",
"cov" (n, 6: c00 c01 c02 c11 c12 c22, the covariance the solver saw), and "sweeps", the number of Jacobi sweeps that got past the all-zero
test."""
import ctypes
import ctypes.util

import numpy as np

NAMES = ["eigenvalue_1", "eigenvalue_2", "eigenvalue_3", "linearity", "planarity", "scattering", "anisotropy", "surface_variation", "eigenvalue_sum",
         "verticality", "omnivariance", "eigenentropy", "count"]   # plane t has bit 1 << t
BITS = {name: 1 << t for t, name in enumerate(NAMES)}
ALL = 8191
MAX_SWEEPS = 10
CANONICAL_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cbrt, _libm.log):
    _f.restype = ctypes.c_double
    _f.argtypes = [ctypes.c_double]


def _per_element(fn, a):
    return np.array([fn(float(v)) for v in a], dtype=np.float64).reshape(a.shape)


def valid_slots(pts, knn, max_distance=np.inf):
    """((n, k) bool, (n, k, 3) gathered neighbours): slot t of query q is valid iff its index is in range, the neighbour and the query are
    finite and the slot distance is <= max_distance."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    j = np.asarray(knn).astype(np.int64) & 0xFFFFFFFF        # -1 is the 0xFFFFFFFF padding
    in_range = j < n
    p = pts[np.where(in_range, j, 0)]
    with np.errstate(all="ignore"):
        dx = p[..., 0] - pts[:, None, 0]
        dy = p[..., 1] - pts[:, None, 1]
        dz = p[..., 2] - pts[:, None, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        near = d <= max_distance
    return in_range & np.isfinite(p).all(axis=2) & np.isfinite(pts).all(axis=1)[:, None] & near, p


def _ordered_sum(terms, valid):
    """terms, valid: (n, k).  The valid terms added left to right, starting from the first valid one."""
    s = np.zeros(terms.shape[0])
    started = np.zeros(terms.shape[0], dtype=bool)
    for t in range(terms.shape[1]):
        v = valid[:, t]
        s = np.where(v, np.where(started, s + terms[:, t], terms[:, t]), s)
        started = started | v
    return s


def _rotate(a, V, p, q, r, live):
    """steps 1 - 4 for the pair (p, q) on the neighbourhoods in `live`; a: dict (i, j), i <= j -> array; V: 3 x 3 list of arrays"""
    key = lambda i, j: (i, j) if i <= j else (j, i)  # noqa: E731
    app, aqq, apq, arp, arq = a[(p, p)], a[(q, q)], a[key(p, q)], a[key(r, p)], a[key(r, q)]
    g = np.abs(apq)
    small = (g != 0.0) & (np.abs(app) + g == np.abs(app)) & (np.abs(aqq) + g == np.abs(aqq))
    apq = np.where(live & small, 0.0, apq)
    do = live & (apq != 0.0)
    theta = (aqq - app) / (2.0 * apq)
    t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    a[(p, p)] = np.where(do, app - h, app)
    a[(q, q)] = np.where(do, aqq + h, aqq)
    a[key(p, q)] = np.where(do, 0.0, apq)
    a[key(r, p)] = np.where(do, c * arp - s * arq, arp)
    a[key(r, q)] = np.where(do, s * arp + c * arq, arq)
    for i in range(3):
        vp, vq = V[i][p], V[i][q]
        V[i][p] = np.where(do, c * vp - s * vq, vp)
        V[i][q] = np.where(do, s * vp + c * vq, vq)


def _order_pair(lam, V, i, j):
    """stable descending: exchanged only where the later value is strictly larger"""
    swap = lam[j] > lam[i]
    lam[i], lam[j] = np.where(swap, lam[j], lam[i]), np.where(swap, lam[i], lam[j])
    for row in range(3):
        V[row][i], V[row][j] = np.where(swap, V[row][j], V[row][i]), np.where(swap, V[row][i], V[row][j])


def _oriented(x, y, z):
    flip = (z < 0.0) | ((z == 0.0) & ((y < 0.0) | ((y == 0.0) & (x < 0.0))))
    return np.stack([np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)], axis=1)


def features(pts, knn, max_distance=np.inf):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    n = len(pts)
    valid, p = valid_slots(pts, knn, max_distance)
    m = valid.sum(axis=1)
    md = m.astype(np.float64)
    with np.errstate(all="ignore"):
        c = [_ordered_sum(p[..., a], valid) / md for a in range(3)]
        d = [p[..., a] - c[a][:, None] for a in range(3)]
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        cov = {ij: _ordered_sum(d[ij[0]] * d[ij[1]], valid) / md for ij in pairs}
        scale = np.max(np.abs(np.stack([cov[ij] for ij in pairs])), axis=0)      # a NaN entry makes it a NaN
        solved = (m >= 3) & np.isfinite(scale)
        live = solved & (scale != 0.0)
        a = {ij: np.where(live, cov[ij] / scale, 0.0) for ij in pairs}
        V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
        sweeps = np.zeros(n, dtype=np.int64)
        for _ in range(MAX_SWEEPS):
            live = live & ~((a[(0, 1)] == 0.0) & (a[(0, 2)] == 0.0) & (a[(1, 2)] == 0.0))
            if not live.any():
                break
            sweeps += live
            _rotate(a, V, 0, 1, 2, live)
            _rotate(a, V, 0, 2, 1, live)
            _rotate(a, V, 1, 2, 0, live)
        lam = [np.where(scale != 0.0, a[(i, i)] * scale, 0.0) for i in range(3)]
        _order_pair(lam, V, 0, 1)
        _order_pair(lam, V, 1, 2)
        _order_pair(lam, V, 0, 1)
        l1, l2, l3 = [np.where(v > 0.0, v, 0.0) for v in lam]
        total = (l1 + l2) + l3
        e = [l / total for l in (l1, l2, l3)]
        prod = (e[0] * e[1]) * e[2]
        full = solved & (l1 != 0.0)              # everything is defined
        omni = np.full(n, CANONICAL_NAN)
        omni[full] = _per_element(_libm.cbrt, prod[full])
        h = np.zeros(n)
        for ei in e:
            pos = full & (ei > 0.0)
            term = np.zeros(n)
            term[pos] = ei[pos] * _per_element(_libm.log, ei[pos])
            h = np.where(pos, h - term, h)
        e1 = _oriented(V[0][0], V[1][0], V[2][0])
        e3 = _oriented(V[0][2], V[1][2], V[2][2])
        e2 = np.stack([V[0][1], V[1][1], V[2][1]], axis=1)
        out = {"eigenvalue_1": l1, "eigenvalue_2": l2, "eigenvalue_3": l3, "eigenvalue_sum": total}
        ratios = {"linearity": (l1 - l2) / l1, "planarity": (l2 - l3) / l1, "scattering": l3 / l1, "anisotropy": (l1 - l3) / l1, "surface_variation": l3 / total,
                  "verticality": 1.0 - np.abs(e3[:, 2]), "omnivariance": omni, "eigenentropy": h}
    for name in out:
        out[name] = np.where(solved, out[name], CANONICAL_NAN)
    for name, v in ratios.items():
        out[name] = np.where(full, v, CANONICAL_NAN)
    out["count"] = md
    out["normals"] = np.where(full[:, None], e3, CANONICAL_NAN)
    out["directions"] = np.where(full[:, None], e1, CANONICAL_NAN)
    out["e2"] = np.where(full[:, None], e2, CANONICAL_NAN)
    out["cov"] = np.stack([cov[ij] for ij in pairs], axis=1)
    out["sweeps"] = sweeps
    return out


def planes(result, bits):
    """(planes, n): one plane per set bit, ascending -- the layout of d_out"""
    return np.stack([result[name] for name in NAMES if bits & BITS[name]])


# ---- the cloud families of the tests ---------------------------------------------------------------------------------------------------------

FAMILIES = ["volume", "utm", "plane_axis", "plane_rotated", "line_axis", "line_rotated", "lattice", "tiny", "huge", "k3", "anisotropic"]


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def family(name, n, seed=0):
    """(points the lists are searched on, factor the points are multiplied by afterwards).  The factor is a power of ten far outside the
    range of squared distances, so the neighbours are chosen on the unscaled cloud."""
    rng = np.random.default_rng([seed, FAMILIES.index(name), n])
    u = rng.random((n, 3))
    if name in ("volume", "k3", "tiny", "huge"):
        pts = u * np.array([100.0, 100.0, 30.0])
        return pts, {"tiny": 1e-150, "huge": 1e150}.get(name, 1.0)
    if name == "utm":
        return u * np.array([100.0, 100.0, 30.0]) + np.array([5e5, 5.6e6, 250.0]), 1.0
    if name == "plane_axis":
        pts = u * 50.0
        pts[:, rng.integers(0, 3)] = 7.0
        return pts, 1.0
    if name == "plane_rotated":
        pts = u * 50.0
        pts[:, 2] = 0.0
        return pts @ _rotation(rng).T + 10.0, 1.0
    if name == "line_axis":
        pts = np.zeros((n, 3)) + np.array([3.0, -4.0, 5.0])
        pts[:, rng.integers(0, 3)] = u[:, 0] * 200.0
        return pts, 1.0
    if name == "line_rotated":
        direction = _rotation(rng)[:, 0]
        return (u[:, :1] * 200.0) * direction[None, :] + np.array([1.0, 2.0, 3.0]), 1.0
    if name == "lattice":
        return rng.integers(0, 12, size=(n, 3)).astype(np.float64), 1.0
    if name == "anisotropic":
        return u * np.array([1e3, 1.0, 1e-3]), 1.0   # eigenvalues spread over 10^12
    raise ValueError(name)
