// pasture_amd/csrc/plane_solve.hpp on its own (host only, no HIP): built with the address and undefined-behaviour sanitizers and run by
// tests/test_plane_solve.py.  The minimum-norm solve of the point-to-plane step is checked on known motions of a curved surface, on
// rank-deficient systems written down analytically (parallel normals, a sphere, zero, not finite), the generalised Jacobi solver on random
// symmetric matrices with and without repeated eigenvalues, and Rodrigues' formula over the whole range of angles.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plane_solve.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      ++failures;                                        \
    }                                                    \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {  // xorshift64*, in [-1, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-52 - 1.0;
}

static double det3(const double R[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
static double orthonormality(const double R[9]) {  // largest entry of |R^T R - I|
  double worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += R[3 * k + i] * R[3 * k + j];
      worst = std::fmax(worst, std::fabs(v - (i == j ? 1.0 : 0.0)));
    }
  return worst;
}
static void proper(const double R[9], const char* what) {
  bool finite = true;
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R[i]);
  const double o = orthonormality(R), d = det3(R);
  CHECK(finite, "%s: not finite", what);
  CHECK(o < 1e-14, "%s: R^T R - I = %g", what, o);
  CHECK(std::fabs(d - 1.0) < 1e-14, "%s: det = %.17g", what, d);
}
static bool is_identity(const double R[9], const double t[3]) {
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  bool same = true;
  for (int i = 0; i < 9; ++i) same = same && R[i] == I[i];
  for (int a = 0; a < 3; ++a) same = same && t[a] == 0.0;
  return same;
}

// the sums of the definition from pairs given as (w, n, r)
struct Pairs {
  std::vector<double> w, n, r;  // w, n: 3 per pair
  void add(const double wv[3], const double nv[3], double rv) {
    for (int a = 0; a < 3; ++a) { w.push_back(wv[a]); n.push_back(nv[a]); }
    r.push_back(rv);
  }
  size_t size() const { return r.size(); }
  void row(size_t i, double j[6]) const {
    const double* wv = &w[3 * i];
    const double* nv = &n[3 * i];
    j[0] = wv[1] * nv[2] - wv[2] * nv[1]; j[1] = wv[2] * nv[0] - wv[0] * nv[2]; j[2] = wv[0] * nv[1] - wv[1] * nv[0];
    j[3] = nv[0]; j[4] = nv[1]; j[5] = nv[2];
  }
  void sums(double A21[21], double g[6], double& sum_w2) const {
    for (int k = 0; k < 21; ++k) A21[k] = 0.0;
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
    sum_w2 = 0.0;
    for (size_t i = 0; i < size(); ++i) {
      double j[6];
      row(i, j);
      for (int p = 0, k = 0; p < 6; ++p) {
        for (int q = p; q < 6; ++q, ++k) A21[k] += j[p] * j[q];
        g[p] += j[p] * r[i];
      }
      sum_w2 += w[3 * i] * w[3 * i] + w[3 * i + 1] * w[3 * i + 1] + w[3 * i + 2] * w[3 * i + 2];
    }
  }
};

// points of the saddle z = 0.9 x^2 - 0.7 y^2 + 0.4 x y (in units of `scale`) over [-scale, scale]^2 about their centroid, with their unit
// normals.  The slopes reach 2: the normals span all directions well, so A' is well conditioned (its eigenvalues lie within a factor of about
// 1e2) and a solve loses two or three of f64's sixteen digits, not more.
static void saddle(int count, double scale, std::vector<double>& w, std::vector<double>& n) {
  std::vector<double> q(3 * count);
  double c[3] = {0, 0, 0};
  n.resize(3 * count);
  for (int i = 0; i < count; ++i) {
    const double x = uniform() * scale, y = uniform() * scale;
    q[3 * i] = x; q[3 * i + 1] = y; q[3 * i + 2] = (0.9 * x * x - 0.7 * y * y + 0.4 * x * y) / scale;
    const double fx = (1.8 * x + 0.4 * y) / scale, fy = (-1.4 * y + 0.4 * x) / scale, len = std::sqrt(fx * fx + fy * fy + 1.0);
    n[3 * i] = -fx / len; n[3 * i + 1] = -fy / len; n[3 * i + 2] = 1.0 / len;
    for (int a = 0; a < 3; ++a) c[a] += q[3 * i + a] / count;
  }
  w.resize(3 * count);
  for (int i = 0; i < count; ++i)
    for (int a = 0; a < 3; ++a) w[3 * i + a] = q[3 * i + a] - c[a];
}

static double norm3(const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// r = j . x exactly as the model has it: (omega, tau) must come back to 1e-12 of |x| (in the commensurate units: omega times the cloud's
// radius L), whatever the size of the cloud and of the motion
static void test_known_linear_motions() {
  for (double scale : {1.0, 100.0, 1e4})
    for (double size : {1e-9, 1e-6, 1e-3}) {
      std::vector<double> w, n;
      saddle(400, scale, w, n);
      const double omega[3] = {0.6 * size, -0.3 * size, 0.74 * size}, tau[3] = {0.5 * size * scale, -0.2 * size * scale, 0.8 * size * scale};
      Pairs pairs;
      for (int i = 0; i < 400; ++i) {
        Pairs one;
        one.add(&w[3 * i], &n[3 * i], 0.0);
        double j[6];
        one.row(0, j);
        pairs.add(&w[3 * i], &n[3 * i], (j[0] * omega[0] + j[1] * omega[1] + j[2] * omega[2]) + (j[3] * tau[0] + j[4] * tau[1] + j[5] * tau[2]));
      }
      double A21[21], g[6], sum_w2, got_omega[3], got_tau[3];
      pairs.sums(A21, g, sum_w2);
      const int rank = pst::plane_solve_xi(A21, g, sum_w2, 400.0, got_omega, got_tau);
      CHECK(rank == 6, "saddle: rank %d", rank);
      const double L = std::sqrt(sum_w2 / 400.0);
      double err = 0.0, size_x = 0.0;
      for (int a = 0; a < 3; ++a) {
        err = std::fmax(err, std::fmax(std::fabs(got_omega[a] - omega[a]) * L, std::fabs(got_tau[a] - tau[a])));
        size_x = std::fmax(size_x, std::fmax(std::fabs(omega[a]) * L, std::fabs(tau[a])));
      }
      CHECK(err <= 1e-12 * size_x, "linear motion, scale %g, size %g: error %g of %g", scale, size, err, size_x);
      const double cq[3] = {5.0e5, 5.4e6, 100.0};
      double dR[9], dt[3];
      pst::plane_solve(A21, g, sum_w2, 400.0, cq, dR, dt);
      proper(dR, "known motion");
    }
}

// The targets are the source moved by an exact rotation exp([omega]x) about the centroid: the linear model leaves out the second order, so
// one step is off by a multiple of theta^2 in omega and in tau (printed; about 0.3 theta^2 each on this surface from 1e-6 to 0.1 rad, asserted
// below 2 theta^2); a second step from the moved points squares it again.
static void test_exact_rotations_state_the_linearisation_error() {
  for (double theta : {1e-6, 1e-4, 1e-3, 1e-2, 1e-1}) {
    std::vector<double> w, n;
    saddle(400, 1.0, w, n);
    const double omega[3] = {0.6 * theta, -0.3 * theta, 0.7416198487095663 * theta};
    double R[9];
    pst::rodrigues(omega, R);
    // the source is the inverse rotation of the surface; the pairs are exact, the normals the surface's at the targets
    Pairs pairs;
    for (int i = 0; i < 400; ++i) {
      const double* p = &w[3 * i];
      double q[3];
      for (int a = 0; a < 3; ++a) q[a] = R[a] * p[0] + R[3 + a] * p[1] + R[6 + a] * p[2];  // R^T p
      const double* nv = &n[3 * i];
      pairs.add(q, nv, (p[0] - q[0]) * nv[0] + (p[1] - q[1]) * nv[1] + (p[2] - q[2]) * nv[2]);
    }
    double A21[21], g[6], sum_w2, got_omega[3], got_tau[3];
    pairs.sums(A21, g, sum_w2);
    pst::plane_solve_xi(A21, g, sum_w2, 400.0, got_omega, got_tau);
    const double d[3] = {got_omega[0] - omega[0], got_omega[1] - omega[1], got_omega[2] - omega[2]};
    std::printf("exact rotation of %g rad: omega off by %.3g = %.3g theta^2, tau %.3g\n", theta, norm3(d), norm3(d) / (theta * theta), norm3(got_tau));
    CHECK(norm3(d) <= 2.0 * theta * theta + 1e-12 * theta, "rotation %g: omega off by %g", theta, norm3(d));
    CHECK(norm3(got_tau) <= 2.0 * theta * theta + 1e-12 * theta, "rotation %g: tau %g", theta, norm3(got_tau));
  }
}

static void test_parallel_normals() {
  // every normal (0, 0, 1): j = (w1, -w0, 0, 0, 0, 1); rank 3.  r = lift + tilt: omega_x, omega_y and tau_z come back, omega_z, tau_x, tau_y are 0
  Pairs pairs;
  const double up[3] = {0.0, 0.0, 1.0}, omega_x = 2.5e-3, omega_y = -1.5e-3, lift = 0.125;
  double c[2] = {0, 0};
  std::vector<double> xy(2 * 300);
  for (int i = 0; i < 300; ++i) {
    xy[2 * i] = uniform() * 40.0; xy[2 * i + 1] = uniform() * 25.0;
    c[0] += xy[2 * i] / 300; c[1] += xy[2 * i + 1] / 300;
  }
  for (int i = 0; i < 300; ++i) {
    const double w[3] = {xy[2 * i] - c[0], xy[2 * i + 1] - c[1], 0.0};
    pairs.add(w, up, (w[1] * omega_x - w[0] * omega_y) + lift);
  }
  double A21[21], g[6], sum_w2, omega[3], tau[3];
  pairs.sums(A21, g, sum_w2);
  const int rank = pst::plane_solve_xi(A21, g, sum_w2, 300.0, omega, tau);
  CHECK(rank == 3, "parallel normals: rank %d", rank);
  CHECK(omega[2] == 0.0 && tau[0] == 0.0 && tau[1] == 0.0, "parallel normals: free directions moved: %g %g %g", omega[2], tau[0], tau[1]);
  CHECK(std::fabs(omega[0] - omega_x) <= 1e-12 * std::fabs(omega_x) && std::fabs(omega[1] - omega_y) <= 1e-12 * std::fabs(omega_x) && std::fabs(tau[2] - lift) <= 1e-12 * lift,
        "parallel normals: tilt and lift %.17g %.17g %.17g", omega[0], omega[1], tau[2]);
  const double cq[3] = {5.0e5, 5.4e6, 100.0};
  double dR[9], dt[3];
  pst::plane_solve(A21, g, sum_w2, 300.0, cq, dR, dt);
  proper(dR, "parallel normals");
  // the same plane tilted: the normal (1, 2, 2) / 3 is not an axis, the three free directions are combinations of the unknowns
  Pairs tilted;
  const double nv[3] = {1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0}, e1[3] = {2.0 / 3.0, -2.0 / 3.0, 1.0 / 3.0}, e2[3] = {2.0 / 3.0, 1.0 / 3.0, -2.0 / 3.0};
  for (int i = 0; i < 300; ++i) {
    const double s = xy[2 * i] - c[0], t = xy[2 * i + 1] - c[1];
    const double w[3] = {s * e1[0] + t * e2[0], s * e1[1] + t * e2[1], s * e1[2] + t * e2[2]};
    tilted.add(w, nv, 0.01 * s - 0.02 * t + 0.3);
  }
  tilted.sums(A21, g, sum_w2);
  const int rank2 = pst::plane_solve_xi(A21, g, sum_w2, 300.0, omega, tau);
  CHECK(rank2 == 3, "tilted plane: rank %d", rank2);
  const double L = std::sqrt(sum_w2 / 300.0), size_y = std::fmax(norm3(omega) * L, norm3(tau));
  const double spin = omega[0] * nv[0] + omega[1] * nv[1] + omega[2] * nv[2];                          // rotation about the normal
  const double slide1 = tau[0] * e1[0] + tau[1] * e1[1] + tau[2] * e1[2], slide2 = tau[0] * e2[0] + tau[1] * e2[1] + tau[2] * e2[2];  // in-plane shift
  CHECK(std::fabs(spin) * L <= 1e-15 * size_y * 8 && std::fabs(slide1) <= 1e-15 * size_y * 8 && std::fabs(slide2) <= 1e-15 * size_y * 8,
        "tilted plane: free directions moved: %g %g %g of %g", spin * L, slide1, slide2, size_y);
  CHECK(std::fabs((tau[0] * nv[0] + tau[1] * nv[1] + tau[2] * nv[2]) - 0.3) <= 1e-12, "tilted plane: lift %.17g", tau[0] * nv[0] + tau[1] * nv[1] + tau[2] * nv[2]);
  pst::plane_solve(A21, g, sum_w2, 300.0, cq, dR, dt);
  proper(dR, "tilted plane");
}

static void test_sphere() {
  // normals of a sphere about cq: w = 2 n, so w x n is exactly zero and the rotation block of A is zero: no rotation, the translation is fitted
  Pairs pairs;
  const double shift[3] = {0.03, -0.01, 0.02};
  for (int i = 0; i < 500; ++i) {
    double n[3];
    double len;
    do {
      for (double& a : n) a = uniform();
      len = norm3(n);
    } while (len < 0.1);
    for (double& a : n) a /= len;
    const double w[3] = {2.0 * n[0], 2.0 * n[1], 2.0 * n[2]};
    pairs.add(w, n, n[0] * shift[0] + n[1] * shift[1] + n[2] * shift[2]);
  }
  double A21[21], g[6], sum_w2, omega[3], tau[3];
  pairs.sums(A21, g, sum_w2);
  const int rank = pst::plane_solve_xi(A21, g, sum_w2, 500.0, omega, tau);
  CHECK(rank == 3, "sphere: rank %d", rank);
  CHECK(omega[0] == 0.0 && omega[1] == 0.0 && omega[2] == 0.0, "sphere: rotation %g %g %g", omega[0], omega[1], omega[2]);
  for (int a = 0; a < 3; ++a) CHECK(std::fabs(tau[a] - shift[a]) <= 1e-12 * 0.03, "sphere: tau[%d] = %.17g", a, tau[a]);
  const double cq[3] = {1.0, 2.0, 3.0};
  double dR[9], dt[3];
  pst::plane_solve(A21, g, sum_w2, 500.0, cq, dR, dt);
  proper(dR, "sphere");
  CHECK(dR[0] == 1.0 && dR[4] == 1.0 && dR[8] == 1.0 && dR[1] == 0.0, "sphere: dR is not the identity");
}

static void test_zero_and_non_finite() {
  const double cq[3] = {5.0e5, 5.4e6, 100.0};
  double A21[21] = {0}, g[6] = {0}, dR[9], dt[3];
  pst::plane_solve(A21, g, 0.0, 10.0, cq, dR, dt);
  CHECK(is_identity(dR, dt), "zero A: not the identity");
  g[2] = 1.0;  // a right-hand side with nothing to carry it
  pst::plane_solve(A21, g, 5.0, 10.0, cq, dR, dt);
  CHECK(is_identity(dR, dt), "zero A, g != 0: not the identity");
  for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY})
    for (int at : {0, 7, 20, 21, 26, 27}) {
      double A[21], gg[6] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6};
      for (int k = 0; k < 21; ++k) A[k] = 0.0;
      for (int i = 0, k = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) A[k] = i == j ? 2.0 + i : 0.1;
      double sum_w2 = 40.0;
      if (at < 21) A[at] = bad; else if (at < 27) gg[at - 21] = bad; else sum_w2 = bad;
      pst::plane_solve(A, gg, sum_w2, 10.0, cq, dR, dt);
      proper(dR, "non-finite input");
      if (at < 27) CHECK(is_identity(dR, dt), "non-finite input at %d: not the identity", at);
      for (int a = 0; a < 3; ++a) CHECK(std::isfinite(dt[a]), "non-finite input at %d: dt", at);
    }
  // a negative semi-definite A (not a sum of squares: lambda_max <= 0)
  for (int i = 0, k = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) A21[k] = i == j ? -1.0 : 0.0;
  pst::plane_solve(A21, g, 5.0, 10.0, cq, dR, dt);
  CHECK(is_identity(dR, dt), "negative A: not the identity");
}

template <int N>
static void check_jacobi(double A[N][N], const char* what) {
  double a[N][N], V[N][N], norm = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      a[i][j] = A[i][j];
      norm += A[i][j] * A[i][j];
    }
  norm = std::sqrt(norm);
  pst::jacobi_eigen<N>(a, V);
  double worst_i = 0.0, worst_a = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      double vv = 0.0, vlv = 0.0;
      for (int k = 0; k < N; ++k) {
        vv += V[i][k] * V[j][k];
        vlv += V[i][k] * a[k][k] * V[j][k];
      }
      worst_i = std::fmax(worst_i, std::fabs(vv - (i == j ? 1.0 : 0.0)));
      worst_a = std::fmax(worst_a, std::fabs(vlv - A[i][j]));
    }
  CHECK(worst_i <= 1e-13, "%s: V V^T - I = %g", what, worst_i);
  CHECK(worst_a <= 1e-13 * norm, "%s: V L V^T - A = %g of %g", what, worst_a, norm);
}

static void test_jacobi() {
  for (int round = 0; round < 200; ++round) {
    double A[6][6];
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = uniform() * (round % 3 == 0 ? 1e6 : 1.0);
    check_jacobi<6>(A, "random symmetric");
  }
  // repeated eigenvalues: Q diag(d) Q^T with Q a product of random plane rotations
  const double spectra[4][6] = {{1, 1, 2, 2, 2, 5}, {3, 3, 3, 3, 3, 3}, {0, 0, 0, 1, 1, 4}, {-2, -2, 7, 7, 7, 7}};
  for (int round = 0; round < 40; ++round) {
    double Q[6][6];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) Q[i][j] = i == j ? 1.0 : 0.0;
    for (int rot = 0; rot < 30; ++rot) {
      const int p = (int)((uniform() + 1.0) * 3.0) % 6, q = (p + 1 + (int)((uniform() + 1.0) * 2.5) % 5) % 6;
      const double angle = uniform() * 3.141592653589793, c = std::cos(angle), s = std::sin(angle);
      for (int k = 0; k < 6; ++k) {
        const double a = Q[k][p], b = Q[k][q];
        Q[k][p] = c * a - s * b;
        Q[k][q] = s * a + c * b;
      }
    }
    double A[6][6];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        double v = 0.0;
        for (int k = 0; k < 6; ++k) v += Q[i][k] * spectra[round % 4][k] * Q[j][k];
        A[i][j] = v;
      }
    for (int i = 0; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j) A[j][i] = A[i][j] = 0.5 * (A[i][j] + A[j][i]);
    check_jacobi<6>(A, "repeated eigenvalues");
  }
  double I3[4][4] = {{3, 0, 0, 0}, {0, 3, 0, 0}, {0, 0, 3, 0}, {0, 0, 0, 3}};
  check_jacobi<4>(I3, "a multiple of the identity, N = 4");
}

static void test_rodrigues() {
  for (double theta : {0.0, 1e-300, 1e-160, 1e-20, 1e-9, 1e-4, 0x1p-6 * (1 - 0x1p-52), 0x1p-6, 0.02, 0.5, 1.0, 3.141592653589793, 6.0, 100.0, 1e6}) {
    const double axis[3] = {0.48, -0.6, 0.64};
    const double omega[3] = {axis[0] * theta, axis[1] * theta, axis[2] * theta};
    double R[9];
    pst::rodrigues(omega, R);
    proper(R, "rodrigues");
    // against the axis-angle form
    const double c = std::cos(theta), s = std::sin(theta), k = 1.0 - c, x = axis[0], y = axis[1], z = axis[2];
    const double want[9] = {c + x * x * k, x * y * k - z * s, x * z * k + y * s, y * x * k + z * s, c + y * y * k, y * z * k - x * s, z * x * k - y * s, z * y * k + x * s, c + z * z * k};
    for (int i = 0; i < 9; ++i) CHECK(std::fabs(R[i] - want[i]) <= 2e-15 * std::fmax(1.0, theta), "rodrigues %g: entry %d %.17g vs %.17g", theta, i, R[i], want[i]);
  }
  // the two branches meet: just below and just above the series' limit
  double lo[9], hi[9];
  const double below[3] = {0x1p-6 * (1 - 0x1p-52), 0.0, 0.0}, above[3] = {0x1p-6, 0.0, 0.0};
  pst::rodrigues(below, lo);
  pst::rodrigues(above, hi);
  for (int i = 0; i < 9; ++i) CHECK(std::fabs(lo[i] - hi[i]) <= 4e-16, "rodrigues: the branches differ by %g at entry %d", std::fabs(lo[i] - hi[i]), i);
}

int main() {
  test_known_linear_motions();
  test_exact_rotations_state_the_linearisation_error();
  test_parallel_normals();
  test_sphere();
  test_zero_and_non_finite();
  test_jacobi();
  test_rodrigues();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
