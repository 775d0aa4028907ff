// Height above ground from the k nearest ground points in the XY plane, inverse-squared-distance weighted (include/pasture_amd.h, "Height
// above ground").
//
// Definitions.  G = the points of the ground buffer with three finite components and a non-zero mask byte.  For a finite query q,
// d2(q, p) = dx*dx + dy*dy with dx = p.x - q.x, dy = p.y - q.y; its neighbours are the at most k members of G with the lexicographically
// smallest (d2, ground-buffer index) among those with d2 <= m2.  w_i = 1.0 / d2_i; an exact hit (w_0 not below +inf) gives zg = z_0, else
// num = w_0*z_0 (+ w_i*z_i in order), den = w_0 (+ w_i in order), zg = num / den.  Every operation a separately rounded f64 operation.
//
// The index is rebuilt by every call (hag_api.cpp): G sorted by cell key, key = (cy << bx) | cx with cell = trunc((v - min) / edge) per axis
// over G's AABB in x and y (hag_grid.hpp), x, y, z in that order as three f64 arrays next to the buffer index of every sorted position, and a
// DENSE directory: dir[cy * cols + cx] = the first sorted position whose cell is that one or a later one, dir[cols * rows] = |G|.  The cells
// [x0, x1] of row y are the sorted positions dir[y * cols + x0] .. dir[y * cols + x1 + 1]: two loads where nn.hip pays two binary searches.
//
// The search, one lane per query, one wave per workgroup, queries in cell order (clamped into the AABB and keyed like a ground point, then
// sorted: the lanes of a wave are neighbours and read the same candidates).  A lane visits the 3 x 3 cells around its own (rings 0 and 1 in
// one pass), then ring 2, 3, ..., clipped to the grid: a ring's two face rows are whole ranges, its inner rows their two end cells.  The lane
// keeps its k best (d2, index, sorted position) as a sorted list in LDS, laid out [slot][lane]: a wave's access to one slot is 64 consecutive
// words, and a lane's column sits in the same banks whatever the slot, so lanes at different slots do not conflict either.  Every slot
// starts at (m2, 0xFFFFFFFF) and a candidate enters when it is lexicographically below the LAST slot: the bound, "fewer than k so far" and the
// tie rule are that one compare, and the order in which candidates arrive cannot matter.  The last slot's pair is mirrored in two registers,
// so a candidate that does not enter costs no LDS access.
//
// When the walk may stop: after ring r as soon as last.d2 <= (r * edge_stop)^2, edge_stop = edge * (1 - 2^-20).  It is nn.hip's argument, and
// what changes is this:
//   clamping   unchanged, for x and y: per axis |p - q| >= |p - c| as real numbers for every p of G (z is neither clamped nor looked at).
//   cells      unchanged, with "some axis" now one of TWO: a member of G that rings 0 .. r have not visited is more than r cells from c's
//              cell in x or in y, so |p - c| > r * edge * (1 - 2^-30) on that axis.
//   margin     d2 is one rounded sum of two rounded squares of rounded differences (one sum fewer than in 3-D): at least
//              (r * edge)^2 * (1 - 2^-28), and (r * edge_stop)^2 as computed is below (r * edge)^2 * (1 - 2^-20).
//   kth best   `best_d2` becomes last.d2, the d2 of the k-th best so far (m2 while fewer than k were found): an unvisited p has
//              d2(p) > (r * edge_stop)^2 >= last.d2 STRICTLY, so it is not lexicographically below the last slot -- it can neither enter the
//              list nor tie with its last member, and the k best among the visited points are the k best of G.
//   a dim of 1 still holds: that axis never is "the axis more than r cells away" and the bound rests on the other one; with both dims 1
//              rmax is 0 and the walk ends after the first pass, every cell visited.
//   rmax       the largest cell distance from c's cell to a side of the grid: ring rmax is the last one that holds a cell.
//   the cell of the largest coordinate is dim - 1 by the expression hag_grid.hpp sized dim with: no clamp of a cell number is ever taken.
// The result depends on the two clouds, the mask, k and max_distance alone.  Ring r costs two directory reads per row, O(r) in all (nn.hip:
// O(r^2) binary searches in 3-D), so a query far from any ground -- the middle of a large roof -- is cheap per ring.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kQ = pstk::kHagQueriesPerBlock;
constexpr uint32_t kBP = pstk::kHagBoundsPointsPerBlock;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr double kNaN = __builtin_nan("");
static_assert(kQ == 64, "the search kernel is written for one wave per workgroup");
static_assert(kBP % kBlock == 0, "a thread of the bounds kernel takes kBP / kBlock points");

using Grid = pstk::HagGrid;
using Bounds = pstk::HagBounds;

__device__ __forceinline__ uint32_t cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;  // 0 <= q < 2^21: the conversion truncates
  return c < dim ? c : dim - 1;    // (never taken, see above)
}
__device__ __forceinline__ double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool finite3(double x, double y, double z) { return finite(x) && finite(y) && finite(z); }

// ---- masked 2-D bounds and count of G ---------------------------------------------------------------------------------------------------------
// wave: xor tree; block: the waves' values in wave order.  Valid in thread 0.  Minima and maxima of finite values: the order cannot matter.
__device__ __forceinline__ void block_fold(double (&mn)[2], double (&mx)[2], unsigned long long& c, double* sv, unsigned long long* sc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      mn[a] = fold_min(mn[a], shfl_xor_any(mn[a], off));
      mx[a] = fold_max(mx[a], shfl_xor_any(mx[a], off));
    }
    c = c + shfl_xor_any(c, off);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sv[wave * 4 + 0] = mn[0]; sv[wave * 4 + 1] = mn[1]; sv[wave * 4 + 2] = mx[0]; sv[wave * 4 + 3] = mx[1];
    sc[wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) {
      mn[0] = fold_min(mn[0], sv[w * 4 + 0]); mn[1] = fold_min(mn[1], sv[w * 4 + 1]);
      mx[0] = fold_max(mx[0], sv[w * 4 + 2]); mx[1] = fold_max(mx[1], sv[w * 4 + 3]);
      c = c + sc[w];
    }
  }
}

__global__ __launch_bounds__(kBlock) void hag_bounds_partial_kernel(Pos pos, uint64_t n, const uint8_t* __restrict__ mask, Bounds* __restrict__ partials) {
  __shared__ double sv[(kBlock / 64) * 4];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kBP;
  double mn[2] = {kInf, kInf}, mx[2] = {-kInf, -kInf};
  unsigned long long c = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < kBP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    if (mask && !mask[i]) continue;
    double x, y, z;
    load_point(pos, i, x, y, z);
    if (!finite3(x, y, z)) continue;
    mn[0] = fold_min(mn[0], x); mn[1] = fold_min(mn[1], y);
    mx[0] = fold_max(mx[0], x); mx[1] = fold_max(mx[1], y);
    c += 1;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) partials[blockIdx.x] = Bounds{mn[0], mn[1], mx[0], mx[1], c};
}

// ONE workgroup: thread t folds the contiguous run [t * per, (t + 1) * per) of the block partials, then the same tree
__global__ __launch_bounds__(kBlock) void hag_bounds_final_kernel(const Bounds* __restrict__ partials, uint64_t blocks, Bounds* __restrict__ rec) {
  __shared__ double sv[(kBlock / 64) * 4];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t per = (blocks + kBlock - 1) / kBlock, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double mn[2] = {kInf, kInf}, mx[2] = {-kInf, -kInf};
  unsigned long long c = 0;
  for (uint64_t b = b0; b < b1; ++b) {
    const Bounds p = partials[b];
    mn[0] = fold_min(mn[0], p.min_x); mn[1] = fold_min(mn[1], p.min_y);
    mx[0] = fold_max(mx[0], p.max_x); mx[1] = fold_max(mx[1], p.max_y);
    c = c + p.count;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) *rec = Bounds{mn[0], mn[1], mx[0], mx[1], c};
}

// ---- keys, gather, directory ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hag_ground_key_kernel(Pos pos, uint64_t n, const uint8_t* __restrict__ mask, Grid g, uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t key = 1u << (g.bits[0] + g.bits[1]);  // not in G: behind every member
  if (!mask || mask[i]) {
    double x, y, z;
    load_point(pos, i, x, y, z);
    if (finite3(x, y, z)) key = (cell_of(y, g.min[1], g.edge, g.dim[1]) << g.bits[0]) | cell_of(x, g.min[0], g.edge, g.dim[0]);
  }
  keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void hag_gather_kernel(Pos pos, const uint32_t* __restrict__ order, uint32_t ng, double* __restrict__ xs, double* __restrict__ ys,
                                                            double* __restrict__ zs) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= ng) return;
  double x, y, z;
  load_point(pos, order[s], x, y, z);
  xs[s] = x; ys[s] = y; zs[s] = z;
}

__global__ __launch_bounds__(kBlock) void hag_heads_kernel(const uint32_t* __restrict__ keys, uint32_t ng, uint32_t bx, uint32_t cols, uint32_t cells,
                                                           uint32_t* __restrict__ dir) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s == 0) dir[cells] = ng;
  if (s >= ng) return;
  const uint32_t key = keys[s];
  if (s == 0 || key != keys[s - 1]) dir[(key >> bx) * cols + (key & ((1u << bx) - 1u))] = s;  // (a member of G: cy < rows, cx < cols)
}

__global__ __launch_bounds__(kBlock) void hag_query_key_kernel(Pos pos, uint64_t n, Grid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  load_point(pos, i, x, y, z);
  uint32_t key = 1u << (g.bits[0] + g.bits[1]);  // not finite: behind every finite query
  if (finite3(x, y, z))
    key = (cell_of(clamp(y, g.min[1], g.max[1]), g.min[1], g.edge, g.dim[1]) << g.bits[0]) | cell_of(clamp(x, g.min[0], g.max[0]), g.min[0], g.edge, g.dim[0]);
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// ---- the search -------------------------------------------------------------------------------------------------------------------------------
// A lane's k-best list: column `lane` of three [k][64] arrays in dynamic LDS (d2 | buffer index | sorted position), and the last slot's pair
// in registers.  Only the lane itself reads or writes its column: no barrier is needed.
struct List {
  double* d2;
  uint32_t *idx, *at;
  uint32_t k;
  double last_d2;
  uint32_t last_idx;
};

__device__ __forceinline__ void offer(List& l, double d2, uint32_t j, uint32_t c) {
  uint32_t p = l.k - 1;  // the candidate is below the last slot: that one drops out
  while (p > 0) {
    const double pd = l.d2[(p - 1) * kQ];
    const uint32_t pi = l.idx[(p - 1) * kQ];
    if (!(d2 < pd || (d2 == pd && j < pi))) break;
    l.d2[p * kQ] = pd;
    l.idx[p * kQ] = pi;
    l.at[p * kQ] = l.at[(p - 1) * kQ];
    --p;
  }
  l.d2[p * kQ] = d2;
  l.idx[p * kQ] = j;
  l.at[p * kQ] = c;
  l.last_d2 = l.d2[(l.k - 1) * kQ];
  l.last_idx = l.idx[(l.k - 1) * kQ];
}

__device__ __forceinline__ void scan(const double* __restrict__ xs, const double* __restrict__ ys, const uint32_t* __restrict__ gidx, uint32_t first, uint32_t last, double qx,
                                     double qy, List& l) {
  for (uint32_t c = first; c < last; ++c) {
    const double dx = xs[c] - qx, dy = ys[c] - qy;
    const double d2 = dx * dx + dy * dy;
    if (d2 <= l.last_d2) {
      const uint32_t j = gidx[c];
      if (d2 < l.last_d2 || j < l.last_idx) offer(l, d2, j, c);
    }
  }
}

__global__ __launch_bounds__(kQ) void hag_search_kernel(Pos pos, uint32_t nq, Grid g, uint32_t k, double m2, const uint32_t* __restrict__ qkeys,
                                                        const uint32_t* __restrict__ order, const uint32_t* __restrict__ dir, const double* __restrict__ xs,
                                                        const double* __restrict__ ys, const double* __restrict__ zs, const uint32_t* __restrict__ gidx,
                                                        double* __restrict__ out_hag, double* __restrict__ out_gz, unsigned long long* __restrict__ unresolved) {
  extern __shared__ double lds[];  // k * 64 doubles, then 2 * k * 64 words
  const uint32_t lane = threadIdx.x;
  const uint32_t s = blockIdx.x * kQ + lane;
  bool unres = false;
  if (s < nq) {
    const uint32_t i = order[s];
    const uint32_t key = qkeys[s];
    const uint32_t bx = g.bits[0], by = g.bits[1];
    double zg = kNaN, qz = kNaN;
    if (!(key >> (bx + by))) {  // a finite query
      List l;
      l.d2 = lds + lane;
      l.idx = (uint32_t*)(lds + k * kQ) + lane;
      l.at = l.idx + k * kQ;
      l.k = k;
      for (uint32_t p = 0; p < k; ++p) { l.d2[p * kQ] = m2; l.idx[p * kQ] = kNone; l.at[p * kQ] = kNone; }
      l.last_d2 = m2;
      l.last_idx = kNone;
      double qx, qy;
      load_point(pos, i, qx, qy, qz);
      const uint32_t cols = g.dim[0], rows = g.dim[1];
      const uint32_t cx = key & ((1u << bx) - 1u), cy = key >> bx;
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
            scan(xs, ys, gidx, dir[row + x0], dir[row + x1 + 1], qx, qy, l);
          } else {  // an inner row: the two end cells, where the grid has them
            if (cx >= r) scan(xs, ys, gidx, dir[row + cx - r], dir[row + cx - r + 1], qx, qy, l);
            if (cx + r < cols) scan(xs, ys, gidx, dir[row + cx + r], dir[row + cx + r + 1], qx, qy, l);
          }
        }
        if (r >= rmax) break;
        const double reach = (double)r * g.edge_stop;
        if (l.last_d2 <= reach * reach) break;
      }
      // the neighbours are the slots that hold a ground point: they come first, in the order of the definition
      if (l.idx[0] != kNone) {
        const double z0 = zs[l.at[0]];
        const double w0 = 1.0 / l.d2[0];
        if (!(w0 < kInf)) {
          zg = z0;  // an exact hit
        } else {
          double num = w0 * z0, den = w0;
#pragma unroll 1
          for (uint32_t p = 1; p < k && l.idx[p * kQ] != kNone; ++p) {
            const double w = 1.0 / l.d2[p * kQ];
            num = num + w * zs[l.at[p * kQ]];
            den = den + w;
          }
          zg = num / den;
        }
      } else {
        unres = true;
      }
    }
    if (out_gz) out_gz[i] = zg;
    if (out_hag) out_hag[i] = qz - zg;
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(unres));
  if (lane == 0 && c) atomicAdd(unresolved, c);
}

__global__ __launch_bounds__(kBlock) void hag_fill_kernel(Pos pos, uint64_t n, double* __restrict__ out_hag, double* __restrict__ out_gz,
                                                          unsigned long long* __restrict__ unresolved) {
  __shared__ unsigned long long wave_count[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool unres = false;
  if (i < n) {
    double x, y, z;
    load_point(pos, i, x, y, z);
    unres = finite3(x, y, z);
    if (out_gz) out_gz[i] = kNaN;
    if (out_hag) out_hag[i] = kNaN;
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(unres));
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) total += wave_count[w];
    if (total) atomicAdd(unresolved, total);
  }
}

__global__ __launch_bounds__(kBlock) void u8_equals_mask_kernel(cgptr_t base, uint64_t stride, uint64_t n, uint8_t value, uint8_t* __restrict__ mask) {
  const uint64_t first = (uint64_t)blockIdx.x * pstk::kPmfPointsPerBlock;
#pragma unroll
  for (uint32_t j = 0; j < pstk::kPmfPointsPerBlock / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i < n) mask[i] = *(base + i * stride) == value ? 1 : 0;
  }
}

}  // namespace

namespace pstk {

size_t hag_bounds_partials_bytes(uint64_t n) { return (size_t)(blocks_of(n, kBP) ? blocks_of(n, kBP) : 1u) * sizeof(HagBounds); }

bool hag_bounds(const Positions& ground, const uint8_t* mask, void* partials, HagBounds* rec, hipStream_t stream) {
  const unsigned blocks = blocks_of(ground.n, kBP);
  if (blocks) hipLaunchKernelGGL(hag_bounds_partial_kernel, dim3(blocks), dim3(kBlock), 0, stream, pos_of(ground), ground.n, mask, (HagBounds*)partials);
  hipLaunchKernelGGL(hag_bounds_final_kernel, dim3(1), dim3(kBlock), 0, stream, (const HagBounds*)partials, (uint64_t)blocks, rec);
  return launched();
}

bool hag_ground_keys(const Positions& ground, const uint8_t* mask, const HagGrid& g, uint32_t* keys, hipStream_t stream) {
  hipLaunchKernelGGL(hag_ground_key_kernel, dim3(blocks_of(ground.n, kBlock)), dim3(kBlock), 0, stream, pos_of(ground), ground.n, mask, g, keys);
  return launched();
}

bool hag_gather(const Positions& ground, const uint32_t* order, uint32_t ng, double* xs, double* ys, double* zs, hipStream_t stream) {
  if (ng == 0) return true;
  hipLaunchKernelGGL(hag_gather_kernel, dim3(blocks_of(ng, kBlock)), dim3(kBlock), 0, stream, pos_of(ground), order, ng, xs, ys, zs);
  return launched();
}

bool hag_directory_heads(const uint32_t* sorted_keys, uint32_t ng, const HagGrid& g, uint32_t* dir, hipStream_t stream) {
  const uint32_t cells = g.dim[0] * g.dim[1];  // at most 2^26
  hipLaunchKernelGGL(hag_heads_kernel, dim3(blocks_of(ng ? ng : 1, kBlock)), dim3(kBlock), 0, stream, sorted_keys, ng, g.bits[0], g.dim[0], cells, dir);
  return launched();
}

bool hag_query_keys(const Positions& query, const HagGrid& g, uint32_t* keys, uint32_t* vals, hipStream_t stream) {
  hipLaunchKernelGGL(hag_query_key_kernel, dim3(blocks_of(query.n, kBlock)), dim3(kBlock), 0, stream, pos_of(query), query.n, g, keys, vals);
  return launched();
}

bool hag_search(const Positions& query, const HagGrid& g, uint32_t k, double m2, const uint32_t* query_keys, const uint32_t* query_order, const uint32_t* dir,
                const double* xs, const double* ys, const double* zs, const uint32_t* ground_index, double* hag, double* ground_z, unsigned long long* unresolved,
                hipStream_t stream) {
  if (k == 0 || k > kHagMaxK) return false;  // (the LDS of a workgroup is sized by it)
  const size_t lds_bytes = (size_t)k * kQ * 16;
  hipLaunchKernelGGL(hag_search_kernel, dim3(blocks_of(query.n, kQ)), dim3(kQ), lds_bytes, stream, pos_of(query), (uint32_t)query.n, g, k, m2, query_keys, query_order, dir, xs,
                     ys, zs, ground_index, hag, ground_z, unresolved);
  return launched();
}

bool hag_fill_unresolved(const Positions& query, double* hag, double* ground_z, unsigned long long* unresolved, hipStream_t stream) {
  hipLaunchKernelGGL(hag_fill_kernel, dim3(blocks_of(query.n, kBlock)), dim3(kBlock), 0, stream, pos_of(query), query.n, hag, ground_z, unresolved);
  return launched();
}

bool u8_equals_mask(uint64_t addr, uint64_t stride, uint64_t n, uint8_t value, uint8_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(u8_equals_mask_kernel, dim3(blocks_of(n, kPmfPointsPerBlock)), dim3(kBlock), 0, stream, (cgptr_t)addr, stride, n, value, mask);
  return launched();
}

}  // namespace pstk
