// The rigid update of one point-to-plane ICP step from the sums of the used pairs.  No HIP here and no library: plain f64 on the host
// (nn_api.cpp), and tests/cpp/test_plane_solve.cpp includes this header alone (with rigid_solve.hpp, whose Jacobi solver and compose it uses).
//
// A pair (q', p, n) has the residual r = (p - q') . n.  A small rotation by the vector omega about cq and a translation tau move q' by
// omega x w + tau, w = q' - cq, which changes the residual by -(omega . (w x n) + tau . n) = -(j . x), j = (w x n, n), x = (omega, tau).
// The step minimises sum (r - j . x)^2: the normal equations A x = g with A = sum j j^T (symmetric 6 x 6, positive semi-definite), g = sum j r.
//
// The rows of omega carry a length (|w x n| <= |w| |n|), those of tau do not: with L = sqrt(sum |w|^2 / u), the rms distance of the used
// source points from their centroid, S = diag(1/L, 1/L, 1/L, 1, 1, 1) makes the unknowns y = S^-1 x commensurate, A' = S A S, g' = S g.
// A' = V diag(lambda) V^T by cyclic Jacobi rotations, and
//     y = sum over lambda_i > 2^-30 * lambda_max of v_i (v_i . g') / lambda_i,
// the minimum-norm least-squares solution: a direction the pairs do not constrain (three of them when every normal is parallel, the
// rotations on a sphere about cq, a rotation and a translation on a cylinder) gets NO motion, and nothing is ever divided by a tiny number.
// 2^-30 is a definition: a direction constrained 3e4 times more weakly than the best one (the square root of the ratio) cannot be told
// from the rounding of A at 1e8 pairs.  lambda_max <= 0 or a non-finite A, g or L gives the identity update.
//
// dR = exp([omega]x) by Rodrigues' formula, dR = I + a K + b K^2 with K = [omega]x, a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2,
// theta = |omega|.  b is computed as (sin(theta / 2) / (theta / 2))^2 / 2, which does not cancel; below theta = 2^-6 both come from their
// series up to theta^6, whose first neglected term (theta^8 / 9! < 1e-20) is below the rounding of 1.  I + a K + b K^2 is a rotation for
// every omega when a and b are that pair of functions of theta, so the result is a proper rotation to rounding.
#pragma once
#include <cmath>

#include "rigid_solve.hpp"

namespace pst {

constexpr double kPlaneCutoff = 0x1p-30;         // eigenvalues at or below this share of the largest one are treated as zero
constexpr double kPlaneSeriesBelow = 0x1p-6;     // theta below which sin(theta) / theta and (1 - cos(theta)) / theta^2 come from their series

// dR (row-major) = exp([omega]x)
inline void rodrigues(const double omega[3], double R[9]) {
  const double x = omega[0], y = omega[1], z = omega[2];
  const double t2 = x * x + y * y + z * z, theta = std::sqrt(t2);
  double a, b;
  if (theta < kPlaneSeriesBelow) {
    a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
    b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
  } else {
    const double h = 0.5 * theta, sh = std::sin(h) / h;
    a = std::sin(theta) / theta;
    b = 0.5 * sh * sh;
  }
  R[0] = 1.0 - b * (y * y + z * z); R[1] = b * x * y - a * z;         R[2] = b * x * z + a * y;
  R[3] = b * x * y + a * z;         R[4] = 1.0 - b * (x * x + z * z); R[5] = b * y * z - a * x;
  R[6] = b * x * z - a * y;         R[7] = b * y * z + a * x;         R[8] = 1.0 - b * (x * x + y * y);
}

// The minimum-norm solution x = (omega, tau) of A x = g as defined above.  A21: the upper triangle of A, row-major.  Returns the rank used
// (the number of eigenvalues above the cutoff); 0 with x = 0 when A is zero, not positive or not finite.
inline int plane_solve_xi(const double A21[21], const double g[6], double sum_w2, double u, double omega[3], double tau[3]) {
  for (int a = 0; a < 3; ++a) omega[a] = tau[a] = 0.0;
  double L = std::sqrt(sum_w2 / u);
  if (!(L > 0.0) || !std::isfinite(L)) L = 1.0;
  double s[6];
  for (int i = 0; i < 6; ++i) s[i] = i < 3 ? 1.0 / L : 1.0;
  double M[6][6], gs[6], big = 0.0;
  bool ok = true;
  for (int i = 0, k = 0; i < 6; ++i) {
    gs[i] = s[i] * g[i];
    ok = ok && std::isfinite(gs[i]);
    for (int j = i; j < 6; ++j, ++k) {
      M[i][j] = M[j][i] = (s[i] * A21[k]) * s[j];
      ok = ok && std::isfinite(M[i][j]);
      big = std::fmax(big, std::fabs(M[i][j]));
    }
  }
  if (!ok || !(big > 0.0)) return 0;
  for (int i = 0; i < 6; ++i) {  // A' / big and g' / big have the same solution; the squares in the sweeps stay in range
    gs[i] /= big;
    for (int j = 0; j < 6; ++j) M[i][j] /= big;
  }
  double V[6][6];
  jacobi_eigen<6>(M, V);
  double lmax = 0.0;
  for (int i = 0; i < 6; ++i) lmax = std::fmax(lmax, M[i][i]);
  if (!(lmax > 0.0)) return 0;
  double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int rank = 0;
  for (int i = 0; i < 6; ++i) {
    if (!(M[i][i] > kPlaneCutoff * lmax)) continue;
    double dot = 0.0;
    for (int k = 0; k < 6; ++k) dot += V[k][i] * gs[k];
    const double c = dot / M[i][i];
    for (int k = 0; k < 6; ++k) y[k] += V[k][i] * c;
    ++rank;
  }
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(y[k])) return 0;
  for (int a = 0; a < 3; ++a) {
    omega[a] = y[a] / L;
    tau[a] = y[3 + a];
  }
  return rank;
}

// dR = exp([omega]x) about cq and dt = (cq + tau) - dR cq, the update (dR | dt) of the step
inline void plane_solve(const double A21[21], const double g[6], double sum_w2, double u, const double cq[3], double dR[9], double dt[3]) {
  double omega[3], tau[3];
  plane_solve_xi(A21, g, sum_w2, u, omega, tau);
  rodrigues(omega, dR);
  for (int a = 0; a < 3; ++a) dt[a] = (cq[a] + tau[a]) - ((dR[3 * a] * cq[0] + dR[3 * a + 1] * cq[1]) + dR[3 * a + 2] * cq[2]);
}

}  // namespace pst
