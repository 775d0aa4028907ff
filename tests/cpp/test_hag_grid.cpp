// The grid of pst_height_above_ground_device (pasture_amd/csrc/hag_grid.hpp), host only: built with the address and undefined-behaviour
// sanitizers and run by tests/test_hag_grid.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hag_grid.hpp"

using namespace pstk;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static HagGrid grid(double x0, double y0, double x1, double y1, double edge) {
  HagGrid g{};
  CHECK(hag_make_grid(x0, y0, x1, y1, edge, &g));
  return g;
}

// what every grid must satisfy: the limits, the bits, the largest coordinate in the last cell, edge_stop
static void check_invariants(const HagGrid& g) {
  CHECK(g.dim[0] >= 1 && g.dim[0] <= kHagMaxCellsPerAxis && g.dim[1] >= 1 && g.dim[1] <= kHagMaxCellsPerAxis);
  CHECK((uint64_t)g.dim[0] * g.dim[1] <= kHagMaxCells);
  for (int a = 0; a < 2; ++a) {
    CHECK((1ull << g.bits[a]) >= g.dim[a]);
    CHECK(g.bits[a] == 0 || (1ull << (g.bits[a] - 1)) < g.dim[a]);
    CHECK((uint32_t)((g.max[a] - g.min[a]) / g.edge) == g.dim[a] - 1);  // unclamped: the largest coordinate lands in cell dim - 1
    CHECK(hag_cell_of(g.max[a], g.min[a], g.edge, g.dim[a]) == g.dim[a] - 1);
    CHECK(hag_cell_of(g.min[a], g.min[a], g.edge, g.dim[a]) == 0);
  }
  CHECK(g.bits[0] + g.bits[1] <= 27);
  CHECK(g.edge_stop == g.edge * (1.0 - 0x1p-20));
}

int main() {
  {  // a single point: one cell, no bits, the automatic edge is 1
    const double e = hag_auto_edge(1, 0.0, 0.0, 10);
    CHECK(e == 1.0);
    const HagGrid g = grid(5.0, -3.0, 5.0, -3.0, e);
    CHECK(g.dim[0] == 1 && g.dim[1] == 1 && g.bits[0] == 0 && g.bits[1] == 0 && g.edge == 1.0);
    check_invariants(g);
  }
  {  // zero extent in x: one column; the guess comes from y alone, 3 * edge * n / extent = 2k
    const double e = hag_auto_edge(1000, 0.0, 100.0, 3);
    CHECK(e == 2.0 * 3 * 100.0 / (3.0 * 1000.0));
    const HagGrid g = grid(7.0, 0.0, 7.0, 100.0, e);
    CHECK(g.dim[0] == 1 && g.bits[0] == 0 && g.dim[1] == (uint32_t)(100.0 / e) + 1 && g.edge == e);
    check_invariants(g);
  }
  {  // zero extent in y
    const double e = hag_auto_edge(1000, 50.0, 0.0, 1);
    CHECK(e == 2.0 * 50.0 / (3.0 * 1000.0));
    const HagGrid g = grid(0.0, 1.0, 50.0, 1.0, e);
    CHECK(g.dim[1] == 1 && g.bits[1] == 0 && g.dim[0] == (uint32_t)(50.0 / e) + 1);
    check_invariants(g);
  }
  {  // both axes: 9 * edge^2 * n / area = 2k, to rounding
    const double e = hag_auto_edge(100000, 100.0, 400.0, 10);
    const double held = 9.0 * e * e * 100000.0 / (100.0 * 400.0);
    CHECK(std::fabs(held - 20.0) < 1e-9);
    check_invariants(grid(0.0, 0.0, 100.0, 400.0, e));
    // (extents whose product overflows are still a finite guess)
    const double big = hag_auto_edge(1000, 1e200, 1e200, 1);
    CHECK(std::isfinite(big) && big > 0.0);
  }
  {  // a given edge is kept as given when it fits
    const HagGrid g = grid(-10.0, -10.0, 10.0, 30.0, 0.37);
    CHECK(g.edge == 0.37 && g.dim[0] == (uint32_t)(20.0 / 0.37) + 1 && g.dim[1] == (uint32_t)(40.0 / 0.37) + 1);
    check_invariants(g);
    const HagGrid whole = grid(-10.0, -10.0, 10.0, 30.0, 1000.0);  // larger than the AABB: a single cell
    CHECK(whole.edge == 1000.0 && whole.dim[0] == 1 && whole.dim[1] == 1);
    check_invariants(whole);
  }
  {  // the per-axis limit forces the doubling: 2^22 cells along x at edge 1 -> edge 4 (2^21 cells is still one too many)
    const HagGrid g = grid(0.0, 0.0, 4194304.0, 0.0, 1.0);
    CHECK(g.edge == 4.0 && g.dim[0] == (1u << 20) + 1 && g.dim[1] == 1);
    check_invariants(g);
    const HagGrid y = grid(0.0, 0.0, 0.0, 4194304.0, 1.0);
    CHECK(y.edge == 4.0 && y.dim[1] == (1u << 20) + 1 && y.dim[0] == 1);
    check_invariants(y);
  }
  {  // the cell limit forces it: 16384 x 16384 cells at edge 1 is 2^28 -> edge 2 gives (8192 + 1)^2 > 2^26 -> edge 4
    const HagGrid g = grid(0.0, 0.0, 16384.0, 16384.0, 1.0);
    CHECK(g.edge == 4.0 && g.dim[0] == 4097 && g.dim[1] == 4097);
    check_invariants(g);
    const HagGrid fits = grid(0.0, 0.0, 8191.0, 8191.0, 1.0);  // 8192 x 8192 = 2^26 exactly: kept
    CHECK(fits.edge == 1.0 && fits.dim[0] == 8192 && fits.dim[1] == 8192 && fits.bits[0] == 13 && fits.bits[1] == 13);
    check_invariants(fits);
  }
  {  // a tiny given edge on a large extent, and an extent that overflows
    const HagGrid g = grid(-1e9, -1e9, 1e9, 1e9, 1e-300);
    check_invariants(g);
    HagGrid none{};
    CHECK(!hag_make_grid(-1.7e308, 0.0, 1.7e308, 1.0, 1.0, &none));
  }
  {  // the largest coordinate lands in cell dim - 1 for awkward quotients
    const double mins[] = {0.0, -1.0 / 3.0, 1e6 + 0.1, -123456.789};
    const double exts[] = {1.0, 0.3, 0.1 * 3.0, 1000.0 / 7.0, 999.9999999999999};
    const double edges[] = {0.1, 1.0 / 3.0, 0.01, 1.0, 0.7};
    for (double mn : mins)
      for (double ex : exts)
        for (double ed : edges) check_invariants(grid(mn, mn, mn + ex, mn + ex / 2.0, ed));
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
