// The window of the local-maximum filter (pst_tree_tops_device): its radius from a height, and the cells of the candidate grid it can touch.
// No HIP here: trees.hip evaluates these per candidate, trees_api.cpp on the host, and tests/cpp/test_trees_window.cpp includes this header
// alone.  Every operation is a separately rounded f64 operation.
//
// The predicate (include/pasture_amd.h, "Individual trees"): j is in i's window iff fl(fl(dx*dx) + fl(dy*dy)) <= fl(r*r), dx = fl(x_j - x_i),
// dy = fl(y_j - y_i).  Which x_j can pass it, with u = 2^-53:
//   1. fl is monotone and fl(dy*dy) >= 0, so fl(dx*dx) <= fl(dx*dx + dy*dy) <= fl(r*r).
//   2. Normal range: dx*dx * (1 - u) <= fl(dx*dx) and fl(r*r) <= r*r * (1 + u), so |dx| <= r * sqrt((1 + u) / (1 - u)) < r * (1 + 2^-51).
//      Subnormal range: either product is off by at most 2^-1075 absolutely, so dx*dx <= r*r + 2^-1074 and |dx| <= r + 2^-537.
//      fl(r*r) = +inf accepts every j (r need not be infinite for that): the reach is +inf.
//   3. dx = fl(x_j - x_i): |x_j - x_i| <= |dx| / (1 - u) (exact when the difference is subnormal).
//   Together |x_j - x_i| <= reach(r) = r * (1 + 2^-40) + 2^-536 with room to spare: 2^-40 is a power of two far above the 2^-51 + 2^-52 the
//   steps need and far below anything that would widen a box by a cell; it is not a tuned figure.
//   4. x_j is a double and x_j <= x_i + reach as real numbers, so x_j <= fl(x_i + reach): rounding to nearest is monotone and x_j rounds to
//      itself.  Likewise x_j >= fl(x_i - reach).  No further margin is needed for the two sums.
//   5. The cell expression of hag_grid.hpp, trunc(fl(fl(v - min) / edge)), is monotone in v, and every candidate lies in [min, max] of the
//      grid, so cell(x_j) lies between the cells of the two ends clamped into [min, max].  The same along y.
// So the box covers every cell that holds a point the rounded predicate accepts, whatever the edge: the result cannot depend on the grid.
#pragma once
#include <cstdint>

#include "hag_grid.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define PST_TREES_HD __host__ __device__ inline
#else
#define PST_TREES_HD inline
#endif

namespace pstk {

struct TreeWindow { double a, b, r_min, r_max; };   // radii: r = min(max(a + b*h, r_min), r_max)
struct TreeCellBox { uint32_t x0, x1, y0, y1; };    // inclusive cell ranges

constexpr double kTreesReachRel = 0x1p-40;   // step 2 and 3 above need 2^-51 + 2^-52
constexpr double kTreesReachAbs = 0x1p-536;  // the subnormal range of step 2

// a, b, h finite, 0 <= r_min <= r_max: the result is in [r_min, r_max], never a NaN
PST_TREES_HD double trees_window_radius(const TreeWindow& w, double h) {
  const double bh = w.b * h;
  double r = w.a + bh;
  r = r > w.r_min ? r : w.r_min;
  r = r < w.r_max ? r : w.r_max;
  return r;
}

PST_TREES_HD double trees_window_reach(double r) {
  const double r2 = r * r;
  if (!(r2 < __builtin_huge_val())) return __builtin_huge_val();
  const double pad = r * kTreesReachRel;
  return (r + pad) + kTreesReachAbs;
}

// the cells of one axis that values in [v - reach, v + reach] (and in [mn, mx], where every indexed point is) can have; mn <= v <= mx
PST_TREES_HD void trees_axis_cells(double v, double reach, double mn, double mx, double edge, uint32_t dim, uint32_t& c0, uint32_t& c1) {
  double lo = v - reach, hi = v + reach;
  lo = lo > mn ? lo : mn;  // (-inf, or below the grid: its first cell)
  hi = hi < mx ? hi : mx;
  const double q0 = (lo - mn) / edge, q1 = (hi - mn) / edge;
  c0 = (uint32_t)q0;
  c1 = (uint32_t)q1;
  c0 = c0 < dim ? c0 : dim - 1;  // (never taken: hag_grid.hpp sized dim by this expression at mx)
  c1 = c1 < dim ? c1 : dim - 1;
}

PST_TREES_HD TreeCellBox trees_window_cells(double x, double y, double r, const HagGrid& g) {
  const double reach = trees_window_reach(r);
  TreeCellBox b;
  trees_axis_cells(x, reach, g.min[0], g.max[0], g.edge, g.dim[0], b.x0, b.x1);
  trees_axis_cells(y, reach, g.min[1], g.max[1], g.edge, g.dim[1], b.y0, b.y1);
  return b;
}

}  // namespace pstk
