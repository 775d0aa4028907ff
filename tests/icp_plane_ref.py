"""The point-to-plane ICP step restated in numpy (the definition of include/pasture_amd.h, "Nearest neighbours between two clouds, ICP", plane
step), on top of nn_ref.nearest, nn_ref.apply_transform and nn_ref.compose.

Every term is computed with the separately rounded f64 operations of the definition, in its order (numpy evaluates the expressions exactly
so); the sums are taken by math.fsum, so only the order of summation differs from the device.  The solve is numpy.linalg.eigh on A' with the
definition's cutoff, and Rodrigues' formula in numpy: it shares nothing with pasture_amd/csrc/plane_solve.hpp but the definition."""
import math

import numpy as np

import nn_ref as R

CUTOFF = 2.0 ** -30
# positions of the upper triangle of a 6 x 6, row-major: A21[k] = A[I[k], K[k]]
I, K = np.triu_indices(6)


def _fsum_columns(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([math.fsum(col) for col in a.reshape(len(a), -1).T])


def full(A21):
    """The symmetric 6 x 6 of the 21 entries"""
    A = np.zeros((6, 6))
    A[I, K] = A21
    A[K, I] = A21
    return A


def rodrigues(omega):
    """exp([omega]x)"""
    omega = np.asarray(omega, dtype=np.float64)
    theta = math.sqrt(float(omega @ omega))
    Kx = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if theta < 1e-4:  # sin(t)/t = 1 - t^2/6 + O(t^4), (1 - cos t)/t^2 = 1/2 - t^2/24 + O(t^4): the O(t^4) terms are below 1e-17
        a, b = 1.0 - theta * theta / 6.0, 0.5 - theta * theta / 24.0
    else:
        a, b = math.sin(theta) / theta, 2.0 * math.sin(0.5 * theta) ** 2 / (theta * theta)
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def solve(A21, g, sum_w2, u, cq):
    """(omega, tau, dR, dt) of the definition: the minimum-norm solution through numpy's eigh of A' = S A S."""
    omega, tau = np.zeros(3), np.zeros(3)
    with np.errstate(all="ignore"):
        L = math.sqrt(sum_w2 / u) if u > 0 and sum_w2 >= 0 else 1.0
        if not (L > 0.0 and math.isfinite(L)):
            L = 1.0
        S = np.diag([1.0 / L] * 3 + [1.0] * 3)
        A, gs = S @ full(A21) @ S, S @ np.asarray(g, dtype=np.float64)
        if np.all(np.isfinite(A)) and np.all(np.isfinite(gs)):
            lam, V = np.linalg.eigh(A)
            if lam.max() > 0.0:
                keep = lam > CUTOFF * lam.max()
                y = V[:, keep] @ ((V[:, keep].T @ gs) / lam[keep])
                omega, tau = y[:3] / L, y[3:]
    dR = rodrigues(omega)
    cq = np.asarray(cq, dtype=np.float64)
    return omega, tau, dR, (cq + tau) - dR @ cq


def step(query, target, normals, T, max_distance, origin=None, idx=None, cq=None):
    """One point-to-plane step of the definition with T_in = T; `normals` are the target's, in target order.  Returns a dict: m, u; the sums cq,
    A (21), g (6), sum_r2, sum_w2, sum_d2 (fsum accuracy); abs = the sum of the absolute values of the terms of each of those sums (for cq the
    terms (q' - o) / u); omega, tau, dR, dt, T_out, rms.  origin: the o of the first pass (default: the finite targets' minimum, the index's
    grid origin).  cq: evaluate the second pass at THIS centroid instead of the first pass's own (the device's, bit for bit: then only the order
    of summation differs)."""
    q, p, nrm = R.apply_transform(query, T), R._points(target), R._points(normals)
    if idx is None:
        idx, _ = R.nearest(query, target, max_distance, T)
    sel = np.flatnonzero(idx != R.NONE)
    out = {"m": len(sel), "idx": idx, "u": 0}
    if not len(sel):
        return out
    n_all = nrm[idx[sel]]
    with np.errstate(all="ignore"):
        len2 = (n_all[:, 0] * n_all[:, 0] + n_all[:, 1] * n_all[:, 1]) + n_all[:, 2] * n_all[:, 2]
        used = np.isfinite(n_all).all(axis=1) & (len2 > 0.0)
    sel = sel[used]
    u = len(sel)
    out["u"] = u
    if u == 0:
        return out
    o = p[np.isfinite(p).all(axis=1)].min(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
    qm, pm, n = q[sel], p[idx[sel]], nrm[idx[sel]]
    own_cq = o + _fsum_columns(qm - o) / u
    d2 = R.squared_distances(qm, pm)
    centre = own_cq if cq is None else np.asarray(cq, dtype=np.float64)
    w = qm - centre
    a = np.stack([w[:, 1] * n[:, 2] - w[:, 2] * n[:, 1], w[:, 2] * n[:, 0] - w[:, 0] * n[:, 2], w[:, 0] * n[:, 1] - w[:, 1] * n[:, 0]], axis=1)
    d = pm - qm
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    j = np.concatenate([a, n], axis=1)
    terms_A = j[:, I] * j[:, K]
    terms_g = j * r[:, None]
    r2 = r * r
    w2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    A21, g = _fsum_columns(terms_A), _fsum_columns(terms_g)
    sum_r2, sum_w2, sum_d2 = math.fsum(r2), math.fsum(w2), math.fsum(d2)
    omega, tau, dR, dt = solve(A21, g, sum_w2, u, centre)
    out.update(cq=own_cq, A=A21, g=g, sum_r2=sum_r2, sum_w2=sum_w2, sum_d2=sum_d2, omega=omega, tau=tau, dR=dR, dt=dt, T_out=R.compose(dR, dt, T),
               rms=math.sqrt(sum_r2 / u),
               abs={"cq": _fsum_columns(np.abs(qm - o)) / u, "A": _fsum_columns(np.abs(terms_A)), "g": _fsum_columns(np.abs(terms_g)), "sum_r2": math.fsum(np.abs(r2)),
                    "sum_w2": math.fsum(np.abs(w2)), "sum_d2": math.fsum(np.abs(d2))})
    return out


def sums35(s):
    """The step's result in the layout of pst_icp_plane_step's sums[35]"""
    return np.concatenate([[s["m"], s["u"]], s["cq"], s["A"], s["g"], [s["sum_r2"], s["sum_w2"], s["sum_d2"]]])
