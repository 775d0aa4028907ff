// pasture_amd/csrc/rigid_solve.hpp on its own (host only, no HIP): built with the address and undefined-behaviour sanitizers and run by
// tests/test_rigid_solve.py.  The rotation that maximises trace(R H) is checked against known rotations, against degenerate H (reflected pair
// sets, rank 1, rank 0: still a proper rotation) and, for random H, against random rotations: none may reach a larger trace.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rigid_solve.hpp"

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

static void axis_angle(const double axis[3], double angle, double R[9]) {
  const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  const double x = axis[0] / n, y = axis[1] / n, z = axis[2] / n, c = std::cos(angle), s = std::sin(angle), k = 1.0 - c;
  const double r[9] = {c + x * x * k, x * y * k - z * s, x * z * k + y * s, y * x * k + z * s, c + y * y * k, y * z * k - x * s, z * x * k - y * s, z * y * k + x * s, c + z * z * k};
  for (int i = 0; i < 9; ++i) R[i] = r[i];
}
static void random_rotation(double R[9]) {
  double axis[3];
  do {
    for (double& a : axis) a = uniform();
  } while (axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2] < 1e-3);
  axis_angle(axis, uniform() * 3.141592653589793, R);
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
static double trace_RH(const double R[9], const double H[9]) {
  double t = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) t += R[3 * i + k] * H[3 * k + i];
  return t;
}
static bool proper(const double R[9], const char* what) {
  bool finite = true;
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R[i]);
  const double o = orthonormality(R), d = det3(R);
  CHECK(finite, "%s: not finite", what);
  CHECK(o < 1e-14, "%s: R^T R - I = %g", what, o);
  CHECK(std::fabs(d - 1.0) < 1e-14, "%s: det = %.17g", what, d);
  return finite && o < 1e-14 && std::fabs(d - 1.0) < 1e-14;
}

// H = sum (q - cq)(p - cp)^T for p = S q + shift, over a fixed set of points q; S any 3 x 3 matrix
static void pairs_H(const double S[9], const double shift[3], double H[9], double cq[3], double cp[3]) {
  const int n = 12;
  double q[n][3], p[n][3];
  for (int i = 0; i < n; ++i) {
    for (int a = 0; a < 3; ++a) q[i][a] = 10.0 * uniform();
    for (int a = 0; a < 3; ++a) p[i][a] = S[3 * a] * q[i][0] + S[3 * a + 1] * q[i][1] + S[3 * a + 2] * q[i][2] + shift[a];
  }
  for (int a = 0; a < 3; ++a) {
    cq[a] = cp[a] = 0.0;
    for (int i = 0; i < n; ++i) { cq[a] += q[i][a] / n; cp[a] += p[i][a] / n; }
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      H[3 * a + b] = 0.0;
      for (int i = 0; i < n; ++i) H[3 * a + b] += (q[i][a] - cq[a]) * (p[i][b] - cp[b]);
    }
}

static void expect_rotation(const double want[9], const double shift[3], const char* what) {
  double H[9], cq[3], cp[3], R[9], t[3];
  pairs_H(want, shift, H, cq, cp);
  pst::rigid_solve(H, cq, cp, R, t);
  proper(R, what);
  for (int i = 0; i < 9; ++i) CHECK(std::fabs(R[i] - want[i]) < 1e-13, "%s: R[%d] = %.17g, expected %.17g", what, i, R[i], want[i]);
  for (int a = 0; a < 3; ++a) CHECK(std::fabs(t[a] - shift[a]) < 1e-11, "%s: t[%d] = %.17g, expected %.17g", what, a, t[a], shift[a]);
}

int main() {
  const double zero3[3] = {0.0, 0.0, 0.0}, shift[3] = {3.0, -40.0, 0.25};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  expect_rotation(I, zero3, "identity");
  expect_rotation(I, shift, "identity and a translation");
  const double axes[4][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1.0, -2.0, 0.5}};
  const char* names[4] = {"about x", "about y", "about z", "about an oblique axis"};
  const double angles[5] = {0.3, -1.2, 2.9, 3.141592653589793, 1e-9};
  for (int a = 0; a < 4; ++a)
    for (double angle : angles) {
      double R[9];
      axis_angle(axes[a], angle, R);
      expect_rotation(R, shift, names[a]);
    }

  {  // a reflected pair set: the best orthogonal matrix has determinant -1, the result must be the best PROPER rotation
    const double mirror[9] = {1, 0, 0, 0, 1, 0, 0, 0, -1};
    double H[9], cq[3], cp[3], R[9], t[3];
    pairs_H(mirror, shift, H, cq, cp);
    pst::rigid_solve(H, cq, cp, R, t);
    proper(R, "reflected pairs");
    double rot[9];
    for (int k = 0; k < 100; ++k) {
      random_rotation(rot);
      CHECK(trace_RH(R, H) >= trace_RH(rot, H) - 1e-9 * std::fabs(trace_RH(R, H)), "reflected pairs: a random rotation has a larger trace");
    }
  }
  {  // rank 1 (every pair on one line), rank 0 (no spread at all)
    const double line[9] = {2, 0, 0, 0, 0, 0, 0, 0, 0}, none[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double H[9], cq[3], cp[3], R[9], t[3];
    pairs_H(line, shift, H, cq, cp);
    pst::rigid_solve(H, cq, cp, R, t);
    proper(R, "rank 1");
    for (int a = 0; a < 3; ++a) CHECK(std::isfinite(t[a]), "rank 1: t not finite");
    const double oblique[9] = {1, 2, -1, 2, 4, -2, -3, -6, 3};  // u v^T with u = (1, 2, -3), v = (1, 2, -1)
    pst::rigid_solve(oblique, zero3, zero3, R, t);
    proper(R, "rank 1, oblique");
    pst::rigid_solve(none, cq, cp, R, t);
    proper(R, "rank 0");
    for (int i = 0; i < 9; ++i) CHECK(R[i] == I[i], "rank 0: the identity is expected");
    for (int a = 0; a < 3; ++a) CHECK(t[a] == cp[a] - cq[a], "rank 0: t = cp - cq");
    const double tiny[9] = {1e-300, 0, 0, 0, 2e-300, 0, 0, 0, 3e-300}, huge[9] = {1e300, 0, 0, 0, 2e300, 0, 0, 0, 3e299};
    pst::rigid_solve(tiny, zero3, zero3, R, t);
    proper(R, "tiny H");
    pst::rigid_solve(huge, zero3, zero3, R, t);
    proper(R, "huge H");
  }

  // random H: a proper rotation, and no random rotation reaches a larger trace(R H)
  for (int trial = 0; trial < 1000; ++trial) {
    double H[9], R[9], t[3], rot[9];
    const double scale = std::pow(10.0, 6.0 * uniform());
    for (double& h : H) h = scale * uniform();
    pst::rigid_solve(H, zero3, zero3, R, t);
    if (!proper(R, "random H")) break;
    const double best = trace_RH(R, H);
    double size = 0.0;
    for (double h : H) size += std::fabs(h);
    for (int k = 0; k < 100; ++k) {
      random_rotation(rot);
      const double other = trace_RH(rot, H);
      CHECK(best >= other - 1e-13 * size, "random H %d: trace %.17g below a random rotation's %.17g", trial, best, other);
    }
  }

  // composition: (R | t) o T_in
  {
    double R[9], T_in[12], T_out[12];
    const double axis[3] = {0.2, 1.0, -0.4}, t[3] = {1.0, 2.0, 3.0};
    axis_angle(axis, 0.7, R);
    for (int i = 0; i < 12; ++i) T_in[i] = uniform();
    pst::rigid_compose(R, t, T_in, T_out);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 4; ++b) {
        double want = (b == 3 ? t[a] : 0.0);
        for (int k = 0; k < 3; ++k) want += R[3 * a + k] * T_in[4 * k + b];
        CHECK(std::fabs(T_out[4 * a + b] - want) < 1e-15, "compose [%d][%d]", a, b);
      }
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
