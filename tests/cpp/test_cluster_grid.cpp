// The grid of the cluster index (pasture_amd/csrc/cluster_grid.hpp), host only: built with the address and undefined-behaviour sanitizers and
// run by tests/test_cluster_grid.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cluster_grid.hpp"

using namespace pstk;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

struct Box { double min[3], max[3]; };

static ClusterGrid for_tolerance(const Box& b, double tolerance) {
  ClusterGrid g{};
  CHECK(cluster_grid_for_tolerance(b.min, b.max, tolerance, &g));
  return g;
}
static ClusterGrid for_edge(const Box& b, double edge) {
  ClusterGrid g{};
  CHECK(cluster_grid_for_edge(b.min, b.max, edge, &g));
  return g;
}

// what every grid must satisfy: the limit per axis, the bits, the smallest and the largest coordinate in the first and the last cell
static void check_invariants(const ClusterGrid& g, const Box& b) {
  for (int a = 0; a < 3; ++a) {
    CHECK(g.min[a] == b.min[a]);
    CHECK(g.dim[a] >= 1 && g.dim[a] <= kClusterMaxCellsPerAxis);
    if (g.dim[a] == 1) CHECK(g.bits[a] == 0);
    else CHECK(g.dim[a] <= (1ull << g.bits[a]) && (1ull << g.bits[a]) < 2ull * g.dim[a]);
    CHECK((b.max[a] - b.min[a]) / g.edge < (double)kClusterMaxCellsPerAxis);
    CHECK((uint32_t)((b.max[a] - g.min[a]) / g.edge) == g.dim[a] - 1);  // unclamped: the largest coordinate lands in cell dim - 1
    CHECK(cluster_cell_of(b.max[a], g.min[a], g.edge, g.dim[a]) == g.dim[a] - 1);
    CHECK(cluster_cell_of(b.min[a], g.min[a], g.edge, g.dim[a]) == 0);
  }
  CHECK(g.bits[0] + g.bits[1] + g.bits[2] <= 63);
}

int main() {
  const double margin = 1.0 + 0x1p-20;
  CHECK(bits_for(0) == 0 && bits_for(1) == 0 && bits_for(2) == 1 && bits_for(3) == 2 && bits_for(4) == 2 && bits_for(5) == 3);
  CHECK(bits_for(kClusterMaxCellsPerAxis) == 21 && bits_for(1ull << 28) == 28 && bits_for((1ull << 28) + 1) == 29);
  {  // a single point: one cell, no bits
    const Box b{{5.0, -3.0, 0.25}, {5.0, -3.0, 0.25}};
    const ClusterGrid g = for_tolerance(b, 0.5);
    for (int a = 0; a < 3; ++a) CHECK(g.dim[a] == 1 && g.bits[a] == 0);
    CHECK(g.edge == 0.5 * margin);
    check_invariants(g, b);
  }
  {  // zero extent on one axis, and on two: dim 1 there
    const Box sheet{{0.0, 7.0, -10.0}, {100.0, 7.0, 30.0}};
    const ClusterGrid g = for_tolerance(sheet, 1.0);
    CHECK(g.dim[1] == 1 && g.bits[1] == 0);
    CHECK(g.dim[0] == (uint32_t)(100.0 / margin) + 1 && g.dim[2] == (uint32_t)(40.0 / margin) + 1);
    check_invariants(g, sheet);
    const Box rod{{2.0, 7.0, -10.0}, {2.0, 7.0, 30.0}};
    const ClusterGrid h = for_tolerance(rod, 0.125);
    CHECK(h.dim[0] == 1 && h.dim[1] == 1 && h.bits[0] == 0 && h.bits[1] == 0 && h.dim[2] == (uint32_t)(40.0 / (0.125 * margin)) + 1);
    check_invariants(h, rod);
  }
  {  // nothing forces a doubling: the edge is the tolerance times (1 + 2^-20), exactly
    const Box b{{-1.0, -2.0, -3.0}, {9.0, 18.0, 27.0}};
    const double tolerances[] = {0.37, 1.0 / 3.0, 1e-3, 2.5, 1000.0};
    for (double t : tolerances) {
      const ClusterGrid g = for_tolerance(b, t);
      CHECK(g.edge == t * (1.0 + 0x1p-20));
      check_invariants(g, b);
    }
  }
  {  // the quotient extent / edge just below 2^21 - 1: no doubling; at 2^21 - 1: one
    const double limit = (double)kClusterMaxCellsPerAxis;
    for (int axis = 0; axis < 3; ++axis) {
      Box below{{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}}, at = below;
      below.max[axis] = std::nextafter(limit, 0.0);
      at.max[axis] = limit;
      const ClusterGrid g = for_edge(below, 1.0);
      CHECK(g.edge == 1.0 && g.dim[axis] == kClusterMaxCellsPerAxis && g.bits[axis] == 21);
      check_invariants(g, below);
      const ClusterGrid h = for_edge(at, 1.0);
      CHECK(h.edge == 2.0 && h.dim[axis] == (1u << 20) && h.bits[axis] == 20);
      check_invariants(h, at);
    }
    // the same through the tolerance: the quotient is formed with tolerance * (1 + 2^-20)
    const double edge = 0.5 * margin;
    Box below{{0.0, 0.0, 0.0}, {1.0, 1.0, std::nextafter(limit * edge, 0.0)}}, at{{0.0, 0.0, 0.0}, {1.0, 1.0, limit * edge}};
    CHECK(below.max[2] / edge < limit && at.max[2] / edge >= limit);
    CHECK(for_tolerance(below, 0.5).edge == edge);
    CHECK(for_tolerance(at, 0.5).edge == 2.0 * edge);
    check_invariants(for_tolerance(below, 0.5), below);
    check_invariants(for_tolerance(at, 0.5), at);
    // every axis at the limit: 63 key bits, the most there can be
    const Box full{{0.0, 0.0, 0.0}, {below.max[2], below.max[2], below.max[2]}};
    const ClusterGrid f = for_tolerance(full, 0.5);
    CHECK(f.bits[0] + f.bits[1] + f.bits[2] == 63);
    check_invariants(f, full);
  }
  {  // a tiny tolerance on a large extent: many doublings, the limits hold
    const Box b{{-1e9, -1e9, -1e9}, {1e9, 1e9, 2e9}};
    check_invariants(for_tolerance(b, 1e-300), b);
    check_invariants(for_tolerance(b, 1e-6), b);
  }
  {  // the largest coordinate lands in cell dim - 1 for awkward quotients
    const double mins[] = {0.0, -1.0 / 3.0, 1e6 + 0.1, -123456.789};
    const double exts[] = {1.0, 0.3, 0.1 * 3.0, 1000.0 / 7.0, 999.9999999999999};
    const double tolerances[] = {0.1, 1.0 / 3.0, 0.01, 1.0, 0.7};
    for (double mn : mins)
      for (double ex : exts)
        for (double t : tolerances) {
          const Box b{{mn, mn, mn}, {mn + ex, mn + ex / 2.0, mn + ex / 3.0}};
          check_invariants(for_tolerance(b, t), b);
          check_invariants(for_edge(b, t), b);
        }
  }
  {  // an extent that overflows f64 is refused, on any axis, and nothing is written
    for (int axis = 0; axis < 3; ++axis) {
      Box b{{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}};
      b.min[axis] = -1.7e308;
      b.max[axis] = 1.7e308;
      ClusterGrid none{};
      none.edge = -1.0;
      CHECK(!cluster_grid_for_tolerance(b.min, b.max, 1.0, &none));
      CHECK(!cluster_grid_for_edge(b.min, b.max, 1.0, &none));
      CHECK(none.edge == -1.0);
    }
  }
  {  // the given-edge form of the nearest-neighbour index keeps a given edge as given
    const Box b{{-10.0, -10.0, 0.0}, {10.0, 30.0, 5.0}};
    const ClusterGrid g = for_edge(b, 0.37);
    CHECK(g.edge == 0.37 && g.dim[0] == (uint32_t)(20.0 / 0.37) + 1 && g.dim[1] == (uint32_t)(40.0 / 0.37) + 1 && g.dim[2] == (uint32_t)(5.0 / 0.37) + 1);
    check_invariants(g, b);
    const ClusterGrid whole = for_edge(b, 1000.0);  // larger than the AABB: a single cell
    CHECK(whole.edge == 1000.0 && whole.dim[0] == 1 && whole.dim[1] == 1 && whole.dim[2] == 1);
    check_invariants(whole, b);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
