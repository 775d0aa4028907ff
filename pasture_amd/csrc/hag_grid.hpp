// The XY grid of pst_height_above_ground_device, sized on the host.  No HIP here: hag_api.cpp and hag.hip include it through kernels.hpp, and
// tests/cpp/test_hag_grid.cpp includes this header alone.
//
// cell = trunc((v - min) / edge) per axis over the AABB of the ground set G; dim = the cell of the largest coordinate + 1 BY THAT EXPRESSION, so
// that a ground point's cell number is never clamped (hag.hip, "the cell of the largest coordinate").  key = (cy << bits[0]) | cx; the dense
// directory is indexed cy * dim[0] + cx, which orders the cells as the keys do.
#pragma once
#include <cmath>
#include <cstdint>

namespace pstk {

constexpr uint32_t kHagMaxCellsPerAxis = (1u << 21) - 1;  // the ring bound's rounding argument needs quotients below 2^21
constexpr uint64_t kHagMaxCells = 1ull << 26;             // the dense directory: 4 bytes per cell, 256 MiB at the most
constexpr double kHagStopMargin = 0x1p-20;                // edge_stop = edge * (1 - 2^-20)

// min / max: the AABB of G in x and y; dim[0] = cols, dim[1] = rows; every key is below 2^(bits[0] + bits[1])
struct HagGrid { double min[2], max[2]; double edge, edge_stop; uint32_t dim[2]; uint32_t bits[2]; };

inline uint32_t hag_bits_for(uint32_t cells) {
  uint32_t b = 0;
  while ((1ull << b) < cells) ++b;
  return b;
}

// The automatic edge: the 3 x 3 cells around a query hold about 2k ground points if the n points of G filled their rectangle,
// 9 * edge^2 * n / (ex * ey) = 2k.  An axis of zero extent is one layer of cells whatever the edge and is left out: along the other one
// 3 * edge * n / extent = 2k.  No extent at all: one cell, edge 1.  (Square roots per factor: the area itself may overflow.)
inline double hag_auto_edge(uint64_t n, double ex, double ey, uint32_t k) {
  const bool ax = ex > 0.0 && std::isfinite(ex), ay = ey > 0.0 && std::isfinite(ey);
  const double want = 2.0 * (double)k, count = (double)(n ? n : 1);
  double edge = 1.0;
  if (ax && ay) edge = std::sqrt(want / (9.0 * count)) * std::sqrt(ex) * std::sqrt(ey);
  else if (ax || ay) edge = want * (ax ? ex : ey) / (3.0 * count);
  const double longest = std::fmax(ax ? ex : 0.0, ay ? ey : 0.0);
  if (!(edge > longest * 0x1p-40) || !std::isfinite(edge)) edge = longest > 0.0 ? longest * 0x1p-20 : 1.0;
  return edge;
}

// The grid for an edge, given or automatic: the edge is doubled until no axis has more than 2^21 - 1 cells and cols * rows <= 2^26.
// false: the extent of G overflows f64 (nothing is written).
inline bool hag_make_grid(double min_x, double min_y, double max_x, double max_y, double edge, HagGrid* out) {
  HagGrid g{};
  g.min[0] = min_x; g.min[1] = min_y;
  g.max[0] = max_x; g.max[1] = max_y;
  const double extent[2] = {max_x - min_x, max_y - min_y};
  if (!std::isfinite(extent[0]) || !std::isfinite(extent[1])) return false;
  g.edge = edge;
  for (;;) {
    const double qx = extent[0] / g.edge, qy = extent[1] / g.edge;
    if (qx < (double)kHagMaxCellsPerAxis && qy < (double)kHagMaxCellsPerAxis && ((uint64_t)qx + 1) * ((uint64_t)qy + 1) <= kHagMaxCells) break;
    g.edge *= 2.0;
  }
  g.edge_stop = g.edge * (1.0 - kHagStopMargin);
  for (int a = 0; a < 2; ++a) {
    g.dim[a] = (uint32_t)(extent[a] / g.edge) + 1;
    g.bits[a] = hag_bits_for(g.dim[a]);
  }
  *out = g;
  return true;
}

// the expression hag.hip evaluates per point and axis (the host form, for the tests of this header)
inline uint32_t hag_cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;
  return c < dim ? c : dim - 1;
}

}  // namespace pstk
