// The uniform 3-D grid of the cluster index (Euclidean clusters, DBSCAN, Poisson-disk subsampling, the nearest-neighbour index), sized on the
// host.  No HIP here: the API files and the kernels include it through kernels.hpp, and tests/cpp/test_cluster_grid.cpp includes this header
// alone.
//
// cell = trunc((v - min) / edge) per axis over the AABB of the finite points; dim = the cell of the largest coordinate + 1 BY THAT EXPRESSION,
// so that a point's cell number is never clamped.  key = (cz << (bits[0] + bits[1])) | (cy << bits[0]) | cx: 21 key bits per axis at the most,
// 63 in all, and one more bit tells the all-ones key of a non-finite point apart.
#pragma once
#include <cmath>
#include <cstdint>

namespace pstk {

constexpr uint32_t kClusterMaxCellsPerAxis = (1u << 21) - 1;

// dim cells and `bits` key bits per axis (x lowest); every key is below 2^(bits[0] + bits[1] + bits[2])
struct ClusterGrid { double min[3]; double edge; uint32_t dim[3]; uint32_t bits[3]; };

// key bits that hold the cell numbers 0 .. cells - 1
inline uint32_t bits_for(uint64_t cells) {
  uint32_t b = 0;
  while ((1ull << b) < cells) ++b;
  return b;
}

// The grid for a given edge: the edge is doubled until no axis needs more than 2^21 - 1 cells (coarser cells cost pair tests, never
// exactness).  false: the extent of the finite points overflows f64 (nothing is written).
inline bool cluster_grid_for_edge(const double min[3], const double max[3], double edge, ClusterGrid* out) {
  ClusterGrid g{};
  double extent[3];
  for (int a = 0; a < 3; ++a) {
    g.min[a] = min[a];
    extent[a] = max[a] - g.min[a];
    if (!std::isfinite(extent[a])) return false;
  }
  g.edge = edge;
  while (extent[0] / g.edge >= (double)kClusterMaxCellsPerAxis || extent[1] / g.edge >= (double)kClusterMaxCellsPerAxis || extent[2] / g.edge >= (double)kClusterMaxCellsPerAxis)
    g.edge *= 2.0;
  for (int a = 0; a < 3; ++a) {
    g.dim[a] = (uint32_t)(extent[a] / g.edge) + 1;
    g.bits[a] = bits_for(g.dim[a]);
  }
  *out = g;
  return true;
}

// The grid of a search within `tolerance`: the edge is the tolerance times (1 + 2^-20) -- STRICTLY larger, by far more than any rounding of
// the cell numbers (the argument is at the head of clusters.hip) -- and then as above.
inline bool cluster_grid_for_tolerance(const double min[3], const double max[3], double tolerance, ClusterGrid* out) {
  return cluster_grid_for_edge(min, max, tolerance * (1.0 + 0x1p-20), out);
}

// the expression clusters.hip evaluates per point and axis (the host form, for the tests of this header)
inline uint32_t cluster_cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;
  return c < dim ? c : dim - 1;
}

}  // namespace pstk
