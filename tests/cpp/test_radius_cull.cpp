// pasture_amd/csrc/radius_cull.hpp alone, on the CPU (tests/test_radius_cull.py builds this with the address and undefined-behaviour
// sanitizers): the property the radius search's exactness rests on -- every target the rounded predicate accepts lies in a (y, z) row the
// cull keeps and inside the x range it leaves of that row -- over random queries and grids whose edge runs from radius / 8 to 100 radius,
// with dims of 1 on one, two and three axes, a query inside the grid, on a face, outside it and with its ball TANGENT to a cell boundary
// (the case that fails without the cull's margin), on random points of the ball and on an exhaustive lattice of points one and two ulps
// around the sphere's knife edge and around cell boundaries.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "radius_cull.hpp"

using namespace pstk;

static int failures = 0;
static long accepted = 0, tested = 0, rows_kept = 0, rows_seen = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      if (failures < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

static double step(double v, int ulps) {
  for (; ulps > 0; --ulps) v = std::nextafter(v, kInf);
  for (; ulps < 0; ++ulps) v = std::nextafter(v, -kInf);
  return v;
}

// splitmix64: the test's own generator, the same on every machine
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double uniform() {
  uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double)(x >> 11) * 0x1p-53;
}

// the predicate of the definition, one rounding per operation (volatile: no contraction, whatever the flags)
static bool neighbour(const double q[3], double radius, const double p[3]) {
  volatile double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  volatile double dxx = dx * dx, dyy = dy * dy, dzz = dz * dz;
  volatile double s = dxx + dyy;
  volatile double d2 = s + dzz;
  volatile double r2 = radius * radius;
  return d2 <= r2;
}

struct Grid { double min[3], edge; uint32_t dim[3]; };

// the cell of a target, by the expression of the index (nn.hip's cell_of); false: outside the grid, no target can be there
static bool cell_of(const Grid& g, const double p[3], uint32_t c[3]) {
  for (int k = 0; k < 3; ++k) {
    if (!(p[k] >= g.min[k])) return false;
    volatile double d = p[k] - g.min[k];
    volatile double v = d / g.edge;
    if (!(v < (double)g.dim[k])) return false;
    c[k] = (uint32_t)v;
  }
  return true;
}

// p is a possible target: if the predicate accepts it, the cull must keep its cell
static void check_point(const Grid& g, const double q[3], double radius, const double p[3]) {
  uint32_t c[3];
  ++tested;
  if (!cell_of(g, p, c) || !neighbour(q, radius, p)) return;
  ++accepted;
  RadiusBall b;
  const bool any = radius_ball(q, radius, g.min, g.edge, g.dim, b);
  CHECK(any);
  if (!any) return;
  for (int k = 0; k < 3; ++k) CHECK(b.c0[k] <= c[k] && c[k] <= b.c1[k]);
  uint32_t x0 = 1, x1 = 0;
  const bool kept = radius_row_cells(b, c[1], c[2], g.dim[0], x0, x1);
  CHECK(kept);
  if (kept) CHECK(x0 <= c[0] && c[0] <= x1 && x1 < g.dim[0]);
}

// the lattice of points 0, 1 and 2 ulps around p on every axis
static void check_lattice(const Grid& g, const double q[3], double radius, const double p[3]) {
  for (int i = -2; i <= 2; ++i)
    for (int j = -2; j <= 2; ++j)
      for (int k = -2; k <= 2; ++k) {
        const double s[3] = {step(p[0], i), step(p[1], j), step(p[2], k)};
        check_point(g, q, radius, s);
      }
}

static void check_case(const Grid& g, const double q[3], double radius) {
  // the ball's interior and the knife edge in random directions
  for (int t = 0; t < 60; ++t) {
    double d[3], len = 0.0;
    for (int k = 0; k < 3; ++k) { d[k] = 2.0 * uniform() - 1.0; len += d[k] * d[k]; }
    len = std::sqrt(len);
    if (!(len > 1e-3)) continue;
    const double f = uniform();
    const double in[3] = {q[0] + d[0] / len * radius * f, q[1] + d[1] / len * radius * f, q[2] + d[2] / len * radius * f};
    check_point(g, q, radius, in);
    const double on[3] = {q[0] + d[0] / len * radius, q[1] + d[1] / len * radius, q[2] + d[2] / len * radius};
    check_lattice(g, q, radius, on);
  }
  // the knife edge along the axes and the diagonals of the planes and the cube
  for (int sx = -1; sx <= 1; ++sx)
    for (int sy = -1; sy <= 1; ++sy)
      for (int sz = -1; sz <= 1; ++sz) {
        const int nz = (sx != 0) + (sy != 0) + (sz != 0);
        if (nz == 0) continue;
        const double h = radius / std::sqrt((double)nz);
        const double on[3] = {q[0] + sx * h, q[1] + sy * h, q[2] + sz * h};
        check_lattice(g, q, radius, on);
      }
  // cell boundaries: on axis a the coordinate of a boundary near the ball, the other two so that the point lies on the sphere
  for (int a = 0; a < 3; ++a) {
    const double first = std::floor((q[a] - radius - g.min[a]) / g.edge);
    for (int t = 0; t < 12; ++t) {
      const double kcell = first + (double)(long)(uniform() * (2.0 * radius / g.edge + 2.0));
      if (kcell < 0.0 || kcell > (double)g.dim[a]) continue;
      double p[3];
      p[a] = g.min[a] + kcell * g.edge;
      const double da = p[a] - q[a], rest2 = radius * radius - da * da;
      const double rest = rest2 > 0.0 ? std::sqrt(rest2) : 0.0, phi = 6.283185307179586 * uniform();
      p[(a + 1) % 3] = q[(a + 1) % 3] + rest * std::cos(phi);
      p[(a + 2) % 3] = q[(a + 2) % 3] + rest * std::sin(phi);
      check_lattice(g, q, radius, p);
      // and a point of the ball's inside exactly on the boundary
      p[(a + 1) % 3] = q[(a + 1) % 3] + 0.5 * rest * std::cos(phi);
      p[(a + 2) % 3] = q[(a + 2) % 3] + 0.5 * rest * std::sin(phi);
      check_lattice(g, q, radius, p);
    }
  }
  // what the cull leaves of the box (reported, and checked below not to be everything)
  RadiusBall b;
  if (radius_ball(q, radius, g.min, g.edge, g.dim, b))
    for (uint32_t iz = b.c0[2]; iz <= b.c1[2]; ++iz)
      for (uint32_t iy = b.c0[1]; iy <= b.c1[1]; ++iy) {
        uint32_t x0, x1;
        ++rows_seen;
        if (radius_row_cells(b, iy, iz, g.dim[0], x0, x1)) ++rows_kept;
      }
}

static void properties() {
  const double origins[2][3] = {{0.0, 0.0, 0.0}, {5.0e5, 5.4e6, 100.0}};
  const double radii[3] = {0.5, 1.0e-3, 37.25};
  const double edge_factors[6] = {1.0 / 8.0, 1.0 / 3.7, 1.0, 3.1, 17.0, 100.0};
  const uint32_t dims[5][3] = {{24, 24, 24}, {1, 24, 24}, {24, 1, 24}, {24, 1, 1}, {1, 1, 1}};
  for (const auto& origin : origins)
    for (double radius : radii)
      for (double factor : edge_factors)
        for (const auto& dim : dims) {
          Grid g;
          g.edge = radius * factor;
          for (int k = 0; k < 3; ++k) { g.min[k] = origin[k]; g.dim[k] = dim[k]; }
          double ext[3];
          for (int k = 0; k < 3; ++k) ext[k] = g.edge * g.dim[k];
          for (int where = 0; where < 12; ++where) {
            double q[3];
            for (int k = 0; k < 3; ++k) q[k] = g.min[k] + ext[k] * uniform();       // 0: inside
            if (where == 1) q[0] = g.min[0];                                        // on the low x face
            if (where == 2) q[1] = g.min[1] + ext[1];                               // on the high y face
            if (where == 3) q[2] = g.min[2] - 0.75 * radius;                        // outside, within the radius of a face
            if (where == 4) q[0] = g.min[0] + ext[0] + radius * (1.0 - 0x1p-40);    // outside, the ball touches the face
            if (where == 5) q[1] = g.min[1] - 3.0 * radius;                         // outside, farther than the radius
            if (where >= 6) {  // the ball TANGENT to a cell boundary of axis a, from below and from above: the axis' knife edge is the boundary
              const int a = (where - 6) % 3;
              const double boundary = g.min[a] + g.edge * (double)(long)(uniform() * (g.dim[a] + 1));
              q[a] = where < 9 ? boundary - radius : boundary + radius;
            }
            check_case(g, q, radius);
          }
        }
}

static void edges() {
  const double mn[3] = {0.0, 0.0, 0.0};
  const uint32_t dim[3] = {8, 8, 8};
  RadiusBall b;
  // a query farther than the radius from the grid: nothing to search
  const double far_q[3] = {-5.0, 4.0, 4.0};
  CHECK(!radius_ball(far_q, 1.0, mn, 1.0, dim, b));
  const double beyond[3] = {4.0, 4.0, 10.0};
  CHECK(!radius_ball(beyond, 1.0, mn, 1.0, dim, b));
  // the centre of a cell, radius 0.6 cells: the box is three cells wide, the centre row spans three cells, an edge row (gap 0.5, chord
  // sqrt(0.36 - 0.25) = 0.33) keeps its middle cell, the corner rows (gap^2 = 0.5 > 0.36) are gone
  const double mid[3] = {4.5, 4.5, 4.5};
  CHECK(radius_ball(mid, 0.6, mn, 1.0, dim, b));
  CHECK(b.c0[1] == 3 && b.c1[1] == 5 && b.c0[2] == 3 && b.c1[2] == 5);
  uint32_t x0 = 0, x1 = 0;
  CHECK(radius_row_cells(b, 4, 4, 8, x0, x1) && x0 == 3 && x1 == 5);
  CHECK(radius_row_cells(b, 3, 4, 8, x0, x1) && x0 == 4 && x1 == 4);
  CHECK(radius_row_cells(b, 4, 5, 8, x0, x1) && x0 == 4 && x1 == 4);
  CHECK(!radius_row_cells(b, 3, 3, 8, x0, x1) && !radius_row_cells(b, 5, 3, 8, x0, x1));
  // a ball much larger than the grid keeps everything
  CHECK(radius_ball(mid, 100.0, mn, 1.0, dim, b) && b.c0[0] == 0 && b.c1[0] == 7);
  CHECK(radius_row_cells(b, 0, 7, 8, x0, x1) && x0 == 0 && x1 == 7);
  // an overflowing S: NaNs keep rows
  const double huge[3] = {1e308, 4.0, 4.0};
  const double mn_neg[3] = {-1e308, 0.0, 0.0};
  if (radius_ball(huge, 1.0, mn_neg, 1.0, dim, b)) CHECK(radius_row_cells(b, 4, 4, 8, x0, x1) && x0 == 0 && x1 == 7);
}

int main() {
  edges();
  properties();
  std::printf("%ld points tested, %ld accepted by the predicate; the cull kept %ld of %ld box rows\n", tested, accepted, rows_kept, rows_seen);
  CHECK(accepted > 100000);
  CHECK(rows_kept < rows_seen);  // the cull does cut: it is not "keep everything"
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
