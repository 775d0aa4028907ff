// The rigid transform of one ICP step from the sums of the matched pairs.  No HIP here and no library: plain f64 on the host (nn_api.cpp), and
// tests/cpp/test_rigid_solve.cpp includes this header alone.
//
// H = sum (q - cq)(p - cp)^T, H[3 * a + b] = sum (q_a - cq_a) * (p_b - cp_b): q the source points, p their matches.  The rotation R that brings
// the q onto the p in the least-squares sense maximises sum p . (R q) = trace(R H).  Horn's closed form (J. Opt. Soc. Am. A 4, 1987): with the
// unit quaternion u of R, sum p . (R q) = u^T N u for the symmetric 4 x 4 matrix N below, so u is the eigenvector of N's largest eigenvalue.
// Every unit quaternion is a proper rotation: whatever H is -- a reflected pair set, rank 1, all zero -- the result is orthonormal with
// determinant +1, which an SVD needs a sign correction for.  The eigenvectors come from cyclic Jacobi rotations, which keep them orthonormal to
// rounding and converge for every symmetric matrix (equal eigenvalues included: then any vector of the eigenspace is a maximiser).
#pragma once
#include <cmath>

namespace pst {

// Eigen-decomposition of the symmetric N x N matrix a (destroyed: its diagonal ends as the eigenvalues); the columns of v are the eigenvectors.
// (N = 4: Horn's quaternion below; N = 6: the point-to-plane step of plane_solve.hpp.)
template <int N>
inline void jacobi_eigen(double a[N][N], double v[N][N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < N; ++i) {
      diag += a[i][i] * a[i][i];
      for (int j = i + 1; j < N; ++j) off += a[i][j] * a[i][j];
    }
    if (off == 0.0 || off <= 1e-34 * diag) break;  // relative off-diagonal norm below 1e-17: nothing left at f64
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        if (a[p][q] == 0.0) continue;
        // the rotation that annihilates a[p][q] (Golub & Van Loan, symmetric Schur decomposition): t = tan of the smaller angle
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {  // columns p and q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {  // rows p and q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}
inline void jacobi_eigen4(double a[4][4], double v[4][4]) { jacobi_eigen<4>(a, v); }

// R (row-major, proper) maximising trace(R H), and t = cp - R cq.  H need not be finite-safe beyond this: a non-finite H gives the identity.
inline void rigid_solve(const double H[9], const double cq[3], const double cp[3], double R[9], double t[3]) {
  const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double big = 0.0;
  bool ok = true;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      ok = ok && std::isfinite(N[i][j]);
      big = std::fmax(big, std::fabs(N[i][j]));
    }
  double u[4] = {1.0, 0.0, 0.0, 0.0};  // H = 0 (or not finite): every rotation is as good as any other, the identity is returned
  if (ok && big > 0.0) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) N[i][j] /= big;  // the eigenvectors do not depend on the scale; the squares in the sweeps stay in range
    double V[4][4];
    jacobi_eigen4(N, V);
    int best = 0;
    for (int i = 1; i < 4; ++i)
      if (N[i][i] > N[best][best]) best = i;
    double norm = 0.0;
    for (int k = 0; k < 4; ++k) norm += V[k][best] * V[k][best];
    norm = std::sqrt(norm);
    for (int k = 0; k < 4; ++k) u[k] = V[k][best] / norm;
  }
  const double w = u[0], x = u[1], y = u[2], z = u[3];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (y * z + w * x);         R[8] = w * w - x * x - y * y + z * z;
  for (int a = 0; a < 3; ++a) t[a] = cp[a] - ((R[3 * a] * cq[0] + R[3 * a + 1] * cq[1]) + R[3 * a + 2] * cq[2]);
}

// T_out = (R | t) o T_in for row-major 3 x 4 transforms: R_out = R R_in, t_out = R t_in + t
inline void rigid_compose(const double R[9], const double t[3], const double T_in[12], double T_out[12]) {
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 4; ++b) T_out[4 * a + b] = (R[3 * a] * T_in[b] + R[3 * a + 1] * T_in[4 + b]) + R[3 * a + 2] * T_in[8 + b];
    T_out[4 * a + 3] += t[a];
  }
}

}  // namespace pst
