// pasture_amd/csrc/trees_window.hpp alone, on the CPU (tests/test_trees_window.py builds this with the address and undefined-behaviour
// sanitizers): the window radius at its clamps, the cell ranges at the grid's first and last cell and at dims of 1, and the property the
// filter's exactness rests on -- the box covers the cell of EVERY point the rounded predicate accepts -- on an exhaustive lattice of points
// one and two ulps around the knife edge.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "trees_window.hpp"

using namespace pstk;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

static double step(double v, int ulps) {
  for (; ulps > 0; --ulps) v = std::nextafter(v, kInf);
  for (; ulps < 0; ++ulps) v = std::nextafter(v, -kInf);
  return v;
}

// the predicate of the definition, one rounding per operation (volatile: no contraction, whatever the flags)
static bool in_window(double xi, double yi, double r, double xj, double yj) {
  volatile double dx = xj - xi, dy = yj - yi;
  volatile double dxx = dx * dx, dyy = dy * dy;
  volatile double d2 = dxx + dyy;
  volatile double r2 = r * r;
  return d2 <= r2;
}

static void radii() {
  const TreeWindow w{1.5, 0.1, 1.0, 5.0};
  CHECK(trees_window_radius(w, 10.0) == 1.5 + 0.1 * 10.0);
  CHECK(trees_window_radius(w, -100.0) == 1.0);   // the lower clamp
  CHECK(trees_window_radius(w, -5.0) == 1.0);     // exactly at it: a + b*h == r_min
  CHECK(trees_window_radius(w, 35.0) == 5.0);     // exactly at the upper one
  CHECK(trees_window_radius(w, 1e300) == 5.0);
  const TreeWindow down{4.0, -0.25, 0.0, 4.0};    // b < 0: taller trees, smaller windows
  CHECK(trees_window_radius(down, 8.0) == 2.0);
  CHECK(trees_window_radius(down, 16.0) == 0.0);
  CHECK(trees_window_radius(down, 1e6) == 0.0);
  CHECK(trees_window_radius(down, -4.0) == 4.0);
  const TreeWindow open{0.0, 2.0, 0.0, kInf};     // an infinite r_max clamps nothing, and an overflowing product is +inf, not a NaN
  CHECK(trees_window_radius(open, 3.0) == 6.0);
  CHECK(trees_window_radius(open, 1e308) == kInf);
  CHECK(trees_window_radius(open, -1e308) == 0.0);
  const TreeWindow fixed{3.0, 0.0, 3.0, 3.0};     // a fixed window: b = 0
  CHECK(trees_window_radius(fixed, 1e308) == 3.0 && trees_window_radius(fixed, -1e308) == 3.0);
  CHECK(trees_window_reach(0.0) > 0.0 && trees_window_reach(0.0) < 1e-150);
  CHECK(trees_window_reach(3.0) > 3.0 && trees_window_reach(3.0) < 3.0 * (1.0 + 1e-11));
  CHECK(trees_window_reach(kInf) == kInf);
  CHECK(trees_window_reach(1e200) == kInf);       // r*r overflows: the predicate accepts everything
  CHECK(trees_window_reach(1e150) < kInf);
}

static void ranges() {
  HagGrid g{};
  CHECK(hag_make_grid(0.0, 0.0, 100.0, 50.0, 1.0, &g));
  CHECK(g.dim[0] == 101 && g.dim[1] == 51);
  TreeCellBox b = trees_window_cells(0.0, 0.0, 2.5, g);           // the first cell: clipped below
  CHECK(b.x0 == 0 && b.x1 == 2 && b.y0 == 0 && b.y1 == 2);
  b = trees_window_cells(100.0, 50.0, 2.5, g);                   // the last cell: clipped above
  CHECK(b.x0 == 97 && b.x1 == 100 && b.y0 == 47 && b.y1 == 50);
  b = trees_window_cells(50.5, 25.5, 0.25, g);                   // inside one cell
  CHECK(b.x0 == 50 && b.x1 == 50 && b.y0 == 25 && b.y1 == 25);
  b = trees_window_cells(50.5, 25.5, 0.0, g);                    // a radius of 0
  CHECK(b.x0 == 50 && b.x1 == 50 && b.y0 == 25 && b.y1 == 25);
  b = trees_window_cells(50.0, 25.0, 0.0, g);                    // ... on a cell boundary: the reach's absolute term is far below an ulp here
  CHECK(b.x0 == 50 && b.x1 == 50 && b.y0 == 25 && b.y1 == 25);
  b = trees_window_cells(50.5, 25.5, kInf, g);                   // everything
  CHECK(b.x0 == 0 && b.x1 == 100 && b.y0 == 0 && b.y1 == 50);
  b = trees_window_cells(50.5, 25.5, 1e200, g);
  CHECK(b.x0 == 0 && b.x1 == 100 && b.y0 == 0 && b.y1 == 50);
  // dims of 1: one axis, then both
  CHECK(hag_make_grid(5.0, 7.0, 5.0, 20.0, 2.0, &g));
  CHECK(g.dim[0] == 1 && g.dim[1] == 7);
  b = trees_window_cells(5.0, 12.0, 3.0, g);
  CHECK(b.x0 == 0 && b.x1 == 0 && b.y0 == 0 && b.y1 == 4);  // (9 - reach is just below the boundary at 9)
  CHECK(hag_make_grid(5.0, 7.0, 5.0, 7.0, 1.0, &g));
  b = trees_window_cells(5.0, 7.0, 3.0, g);
  CHECK(b.x0 == 0 && b.x1 == 0 && b.y0 == 0 && b.y1 == 0);
  CHECK(hag_make_grid(-3.0, -3.0, 3.0, 3.0, 100.0, &g));         // one cell for everything
  b = trees_window_cells(-1.0, 2.0, 1.0, g);
  CHECK(g.dim[0] == 1 && g.dim[1] == 1 && b.x0 == 0 && b.x1 == 0 && b.y0 == 0 && b.y1 == 0);
}

// every (xj, yj) of the lattice {base + k ulps} x {base + k ulps} that the predicate accepts has its cell inside the box
static long long cover(const HagGrid& g, double xi, double yi, double r, const std::vector<double>& xs, const std::vector<double>& ys) {
  const TreeCellBox b = trees_window_cells(xi, yi, r, g);
  long long accepted = 0;
  for (double xj : xs)
    for (double yj : ys) {
      if (xj < g.min[0] || xj > g.max[0] || yj < g.min[1] || yj > g.max[1]) continue;  // (not an indexed point)
      if (!in_window(xi, yi, r, xj, yj)) continue;
      ++accepted;
      const uint32_t cx = hag_cell_of(xj, g.min[0], g.edge, g.dim[0]), cy = hag_cell_of(yj, g.min[1], g.edge, g.dim[1]);
      if (!(cx >= b.x0 && cx <= b.x1 && cy >= b.y0 && cy <= b.y1)) {
        std::printf("FAILED cover: i (%a, %a) r %a j (%a, %a): cell (%u, %u) outside [%u, %u] x [%u, %u]\n", xi, yi, r, xj, yj, cx, cy, b.x0, b.x1, b.y0, b.y1);
        ++failures;
      }
    }
  return accepted;
}

static void knife_edges() {
  long long accepted = 0;
  const double mins[] = {0.0, -1234.5678, 500000.25};
  const double edges[] = {1.0, 0.3, 1.0 / 3.0, 0.003, 2.5};
  const double radii_[] = {3.0, 0.3, 1.0 / 3.0, 2.5, 0.7071067811865476, 1e-3, 0.0};
  for (double mn : mins)
    for (double edge : edges)
      for (double r : radii_) {
        HagGrid g{};
        CHECK(hag_make_grid(mn, mn, mn + 40.0, mn + 40.0, edge, &g));
        // i on a cell boundary, just beside one, and at an arbitrary place; the window's ends land on and beside boundaries accordingly
        const double at[] = {mn + 12.0 * g.edge, step(mn + 12.0 * g.edge, -1), step(mn + 12.0 * g.edge, 1), mn + 17.123456789, mn, mn + 40.0};
        for (double xi : at)
          for (double yi : {at[0], at[3]}) {
            std::vector<double> xs, ys;
            // around the four ends of the window along each axis, around i itself, and the diagonal ends at r / sqrt(2)
            const double dr[] = {r, -r, 0.0, r * 0.7071067811865476, -r * 0.7071067811865476};
            for (double d : dr)
              for (int u = -2; u <= 2; ++u) {
                xs.push_back(step(xi + d, u));
                ys.push_back(step(yi + d, u));
              }
            accepted += cover(g, xi, yi, r, xs, ys);
          }
      }
  CHECK(accepted > 10000);  // (the lattices do straddle the edge: a test that accepted nothing would prove nothing)
  // one ulp outside fl(x - r): the case the margin exists for.  x_i = 3, r = 3 - 2^-51: fl(x_i - r) is 2^-51 exactly, and a neighbour at
  // x_j = 0 has dx = -3, dx*dx = 9 > fl(r*r) -- rejected -- while r = 3 and x_j = -2^-52 rounds dx to -3 and is ACCEPTED beyond x_i - r.
  HagGrid g{};
  CHECK(hag_make_grid(-1.0, 0.0, 7.0, 1.0, 1.0, &g));
  const double xj = -0x1p-52;
  CHECK(in_window(3.0, 0.0, 3.0, xj, 0.0) && xj < 3.0 - 3.0);
  const TreeCellBox b = trees_window_cells(3.0, 0.0, 3.0, g);
  CHECK(hag_cell_of(xj, g.min[0], g.edge, g.dim[0]) == 0 && b.x0 == 0);  // cell 0 holds it: [-1, 0)
}

int main() {
  radii();
  ranges();
  knife_edges();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
