// The cull of the fixed-radius search (radius.hip): which (y, z) rows of an index's grid, and which cells of a row, can hold a neighbour of a
// query.  No HIP here: radius.hip evaluates these per query and per row, and tests/cpp/test_radius_cull.cpp includes this header alone.
// Every operation is a separately rounded f64 operation.  The argument for the margins is at the head of radius.hip ("Which rows and cells
// may be skipped"); every comparison is written so that a NaN keeps the row.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define PST_RADIUS_HD __host__ __device__ inline
#else
#define PST_RADIUS_HD inline
#endif

namespace pstk {

constexpr double kRadiusPadScale = 0x1p-22;  // m3c2.hip's: pad = 2^-22 * S

// The ball of one query in CELL UNITS of a grid: centre a, padded radius Rp, its square, the pad, and the clamped cell box [c0, c1] per axis.
struct RadiusBall { double a[3], Rp, Rp2, pad; uint32_t c0[3], c1[3]; };

// the cells [lo, hi] of one axis clamped to [0, dim - 1]; false when none is left.  A NaN keeps the whole axis.  (m3c2.hip's clamp_cells)
PST_RADIUS_HD bool radius_clamp_cells(double lo, double hi, uint32_t dim, uint32_t& c0, uint32_t& c1) {
  if (lo >= (double)dim || hi < 0.0) return false;
  c0 = lo > 0.0 ? (uint32_t)lo : 0u;                     // (0 < lo < dim: the conversion truncates)
  c1 = hi < (double)(dim - 1) ? (uint32_t)hi : dim - 1;  // (0 <= hi here, or a NaN, which takes dim - 1)
  return true;
}

// q: the transformed query (finite); false: the ball's box misses the grid, nothing to search
PST_RADIUS_HD bool radius_ball(const double q[3], double radius, const double grid_min[3], double edge, const uint32_t dim[3], RadiusBall& b) {
  double s = 0.0;
  for (int k = 0; k < 3; ++k) {
    b.a[k] = (q[k] - grid_min[k]) / edge;
    s = s + __builtin_fabs(b.a[k]);
  }
  const double Rc = radius / edge;
  const uint32_t dim_max = dim[0] > dim[1] ? (dim[0] > dim[2] ? dim[0] : dim[2]) : (dim[1] > dim[2] ? dim[1] : dim[2]);
  const double S = (s + Rc) + ((double)dim_max + 1.0);
  b.pad = S * kRadiusPadScale;
  b.Rp = Rc + b.pad;
  b.Rp2 = b.Rp * b.Rp;
  for (int k = 0; k < 3; ++k)
    if (!radius_clamp_cells(b.a[k] - b.Rp, b.a[k] + b.Rp, dim[k], b.c0[k], b.c1[k])) return false;
  return true;
}

// distance from v to the interval [c, c + 1] of cell c
PST_RADIUS_HD double radius_cell_gap(double v, uint32_t c) {
  const double lo = (double)c, hi = lo + 1.0;
  return v < lo ? lo - v : (v > hi ? v - hi : 0.0);
}

// the cells x0 .. x1 of row (iy, iz) that can hold a neighbour; false: none
PST_RADIUS_HD bool radius_row_cells(const RadiusBall& b, uint32_t iy, uint32_t iz, uint32_t dimx, uint32_t& x0, uint32_t& x1) {
  const double gy = radius_cell_gap(b.a[1], iy), gz = radius_cell_gap(b.a[2], iz);
  const double g2 = gy * gy + gz * gz;
  if (g2 > b.Rp2) return false;
  const double h2 = b.Rp2 - g2;
  const double h = __builtin_sqrt(h2 > 0.0 ? h2 : 0.0) + b.pad;  // the chord's half length
  const double lo = b.a[0] - h, hi = b.a[0] + h;
  if (!(h == h)) {  // a NaN: the whole row
    x0 = 0; x1 = dimx - 1;
    return true;
  }
  return radius_clamp_cells(lo, hi, dimx, x0, x1);
}

}  // namespace pstk
