// What the kernels over a DENSE 2-D grid share (hag.hip, trees.hip): the cell of a coordinate, the packed key of a member and of a clamped
// query, the ring walk over the dense directory with the argument for when it may stop, and the block fold of the bounds partials.  The
// grid is pstk::HagGrid (hag_grid.hpp); the host side -- keys, sort, directory -- is DenseDirectory (dense_directory.hpp).
//
// The index: the members sorted by cell key, key = (cy << bx) | cx with cell = trunc((v - min) / edge) per axis over the members' AABB in x
// and y, and the directory dir[cy * cols + cx] = the first sorted position whose cell is that one or a later one, dir[cols * rows] = the
// number of members.  The cells [x0, x1] of row y are the sorted positions dir[y * cols + x0] .. dir[y * cols + x1 + 1]: two loads where
// nn.hip pays two binary searches.
//
// The ring walk (walk_rings).  A query c, clamped into the AABB and keyed like a member, visits the 3 x 3 cells around its own (rings 0 and
// 1 in one pass), then ring 2, 3, ..., clipped to the grid: a ring's two face rows are whole ranges, its inner rows their two end cells.
// The caller keeps a bound B = the d2 of the k-th best member so far, which starts at m2, and admits a candidate only when it is
// lexicographically below its k-th best (d2, index).  The walk may stop after ring r as soon as B <= (r * edge_stop)^2, edge_stop = edge *
// (1 - 2^-20).  It is nn.hip's argument, and what changes is this:
//   clamping   unchanged, for x and y: per axis |p - q| >= |p - c| as real numbers for every member p (z is neither clamped nor looked at).
//   cells      unchanged, with "some axis" now one of TWO: a member that rings 0 .. r have not visited is more than r cells from c's cell
//              in x or in y, so |p - c| > r * edge * (1 - 2^-30) on that axis.
//   margin     d2 is one rounded sum of two rounded squares of rounded differences (one sum fewer than in 3-D): at least
//              (r * edge)^2 * (1 - 2^-28), and (r * edge_stop)^2 as computed is below (r * edge)^2 * (1 - 2^-20).
//   kth best   `best_d2` becomes B (m2 while fewer than k were found): an unvisited p has d2(p) > (r * edge_stop)^2 >= B STRICTLY, so it is
//              not lexicographically below the k-th best -- it can neither enter nor tie with it, and the k best among the visited members
//              are the k best of all.
//   a dim of 1 still holds: that axis never is "the axis more than r cells away" and the bound rests on the other one; with both dims 1
//              rmax is 0 and the walk ends after the first pass, every cell visited.
//   rmax       the largest cell distance from c's cell to a side of the grid: ring rmax is the last one that holds a cell.
//   the cell of the largest coordinate is dim - 1 by the expression hag_grid.hpp sized dim with: no clamp of a cell number is ever taken.
// Ring r costs two directory reads per row, O(r) in all (nn.hip: O(r^2) binary searches in 3-D), so a query far from any member -- the
// middle of a large roof -- is cheap per ring.
#pragma once
#include "positions_device.hpp"

namespace pstd {

// the same expression as pstk::hag_cell_of (hag_grid.hpp)
__device__ __forceinline__ uint32_t cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;  // 0 <= q < 2^21: the conversion truncates
  return c < dim ? c : dim - 1;    // (never taken, see above)
}
__device__ __forceinline__ double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- keys -------------------------------------------------------------------------------------------------------------------------------------
// of a member at (x, y), which lies inside the AABB
__device__ __forceinline__ uint32_t member_key(double x, double y, const pstk::HagGrid& g) {
  return (cell_of(y, g.min[1], g.edge, g.dim[1]) << g.bits[0]) | cell_of(x, g.min[0], g.edge, g.dim[0]);
}
// of a query at (x, y), clamped into the AABB first
__device__ __forceinline__ uint32_t query_key(double x, double y, const pstk::HagGrid& g) {
  return member_key(clamp(x, g.min[0], g.max[0]), clamp(y, g.min[1], g.max[1]), g);
}
// of everything else: behind every member or query in the sort
__device__ __forceinline__ uint32_t no_member_key(const pstk::HagGrid& g) { return 1u << (g.bits[0] + g.bits[1]); }
__device__ __forceinline__ bool is_member_key(uint32_t key, const pstk::HagGrid& g) { return !(key >> (g.bits[0] + g.bits[1])); }
// the cell of a member's or a query's key
__device__ __forceinline__ void cell_of_key(uint32_t key, const pstk::HagGrid& g, uint32_t& cx, uint32_t& cy) {
  cx = key & ((1u << g.bits[0]) - 1u);
  cy = key >> g.bits[0];
}

// ---- the ring walk ----------------------------------------------------------------------------------------------------------------------------
// Around the cell (cx, cy).  scan_range(first, last) takes the sorted positions [first, last) of a row's cells; bound() returns B as it stands
// after them.  Inlined with two lambdas, hag_search_kernel (38 VGPRs, 71 SGPRs) and trees_crown_kernel (40, 62) compile to the registers of
// the loop written out in each, no scratch, 8 waves per SIMD -- unlike the 3-D stencil walkers (grid_index_device.hpp).
template <class ScanRange, class Bound>
__device__ __forceinline__ void walk_rings(const pstk::HagGrid& g, const uint32_t* __restrict__ dir, uint32_t cx, uint32_t cy, ScanRange scan_range, Bound bound) {
  const uint32_t cols = g.dim[0], rows = g.dim[1];
  uint32_t rmax = cx > cols - 1 - cx ? cx : cols - 1 - cx;
  rmax = max(rmax, cy > rows - 1 - cy ? cy : rows - 1 - cy);
#pragma unroll 1
  for (uint32_t r = 1;; ++r) {
    const uint32_t y0 = cy >= r ? cy - r : 0, y1 = cy + r < rows ? cy + r : rows - 1;
    const uint32_t x0 = cx >= r ? cx - r : 0, x1 = cx + r < cols ? cx + r : cols - 1;
#pragma unroll 1
    for (uint32_t y = y0; y <= y1; ++y) {
      const uint32_t ay = y > cy ? y - cy : cy - y;
      const uint32_t row = y * cols;  // below 2^26
      if (r == 1 || ay == r) {  // a face row of the ring (ring 1 takes ring 0 along): the whole range
        scan_range(dir[row + x0], dir[row + x1 + 1]);
      } else {  // an inner row: the two end cells, where the grid has them
        if (cx >= r) scan_range(dir[row + cx - r], dir[row + cx - r + 1]);
        if (cx + r < cols) scan_range(dir[row + cx + r], dir[row + cx + r + 1]);
      }
    }
    if (r >= rmax) break;
    const double reach = (double)r * g.edge_stop;
    if (bound() <= reach * reach) break;
  }
}

// ---- the bounds partials ----------------------------------------------------------------------------------------------------------------------
// N minima, N maxima and a count over the workgroup, valid in thread 0: the wave's xor tree, then the waves' values in wave order.  Minima and
// maxima of finite values and an integer sum: the order cannot matter.  sv: 4 * 2 * N doubles, sc: one count per wave.
template <int N>
__device__ __forceinline__ void block_fold(double (&mn)[N], double (&mx)[N], unsigned long long& c, double* sv, unsigned long long* sc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c = c + shfl_xor_any(c, off);
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
  block_reduce_minmax<double, N>(mn, mx, sv);  // (its barrier publishes sc as well)
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) c = c + sc[w];
  }
}

}  // namespace pstd
