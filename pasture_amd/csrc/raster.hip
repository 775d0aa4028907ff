// Rasterisation: per-cell statistics of a cloud on an XY grid, and the hole filler (include/pasture_amd.h, "Rasterisation").
//
// Definitions.  A point's value v is its z, or values[i].  Its cell: qx = (x - x0) / cell, qy = (y - y0) / cell, inside iff 0 <= qx < cols and
// 0 <= qy < rows compared as doubles, then col = (uint32)qx, row = (uint32)qy.  A member: x, y and v finite, a non-zero mask byte, inside.
// Per cell over its members in ascending buffer index: COUNT, MIN / MAX (by the ordered() key: -0.0 below +0.0, a member's bits), MEAN =
// S / m, VARIANCE = SS / m, where every sum is CHUNKED: chunk j = members [256 j, 256 (j + 1)), P_j its left-to-right sum from its first
// element, S = P_0 + P_1 + ... left to right.  SS sums d * d, d = v - MEAN.  Every operation a separately rounded f64 operation.
//
// Two paths (raster_api.cpp chooses), one result:
//   atomic   COUNT, MIN, MAX only.  One pass over the positions: pmf.hip's filtered 64-bit atomicMin on the cell's key, its mirror image for
//            the maximum (a cell's max key only ever INCREASES, so "my key is not above what I read" implies "not above the final maximum"),
//            a 32-bit atomicAdd per member; then one decode pass into the planes.  All three are order-free.
//   sorted   key = row * cols + col (one more bit: not a member), the stable radix sort with the point index as payload -- so a cell's
//            segment is in buffer-index order --, the dense directory (dense_directory.hpp), the values gathered into sorted order, and ONE LANE PER CELL
//            walking its segment: neighbouring lanes read neighbouring segments.  A cell of at most one chunk is all of its sum.  A cell of
//            more is listed and taken by a workgroup: thread t sums chunks t, t + 256, ... each sequentially into scratch, one lane folds the
//            partials in order, and the same again for SS once the mean is known -- the dependent chain of a cell of m members is
//            m / 256 + 256 additions long, not m.
//
// The fill.  One LDS tile of (kPmfTileRows + 2 h) x (kPmfTileCols + 2 h) doubles, lane = column as in pmf.hip's passes: every LDS access of a
// wave is 64 consecutive doubles of one tile row.  An empty output cell visits its square in row-major order.
#include <algorithm>

#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPpb = pstk::kRasterPointsPerBlock;
constexpr uint32_t kChunk = pstk::kRasterChunk;
constexpr uint32_t kTc = pstk::kPmfTileCols, kTr = pstk::kPmfTileRows, kFh = pstk::kRasterFillMaxHalfWidth;
constexpr uint32_t kFillDoubles = (kTr + 2 * kFh) * (kTc + 2 * kFh);
static_assert(kPpb % kBlock == 0, "whole points per lane");
static_assert(kChunk == kBlock, "thread t of the heavy-cell pass owns chunks t, t + kBlock, ...; a light cell is one chunk");
static_assert(kTc == 64 && kBlock == 256 && kTr % (kBlock / 64) == 0, "one wave per tile row, lane = column");
static_assert(kFillDoubles * sizeof(double) <= 48 * 1024, "the LDS budget kRasterFillMaxHalfWidth is chosen from");

using Grid = pstk::PmfGrid;
using Input = pstk::RasterInput;
using Planes = pstk::RasterPlanes;

__device__ __forceinline__ double canonical_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }

// THE member test and cell of a point: both paths call this.  z is loaded only when it is the value.
__device__ __forceinline__ bool member_cell(const Pos& pos, uint64_t i, const Input& in, const Grid& g, uint32_t& cell, double& v) {
  if (in.mask && !in.mask[i]) return false;
  cgptr_t q = pos.base + i * pos.stride;
  const double x = load_un<double>(q), y = load_un<double>(q + 8);
  v = in.values ? in.values[i] : load_un<double>(q + 16);
  if (!(finite(x) && finite(y) && finite(v))) return false;
  const double qx = (x - g.x0) / g.cell, qy = (y - g.y0) / g.cell;
  if (!(qx >= 0.0 && qx < (double)g.cols && qy >= 0.0 && qy < (double)g.rows)) return false;
  cell = (uint32_t)qy * g.cols + (uint32_t)qx;  // below 2^28
  return true;
}

// *total += the workgroup's sum of `mine`: one integer atomic per workgroup
__device__ __forceinline__ void block_count(uint32_t mine, unsigned long long* total) {
  __shared__ uint32_t wave_count[kBlock / 64];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine += shfl_xor_any(mine, off);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) sum += wave_count[w];
    if (sum) atomicAdd(total, sum);
  }
}

__global__ __launch_bounds__(kBlock) void raster_fill_empty_kernel(Planes out, uint64_t n_cells) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cells) return;
  if (out.count) out.count[c] = 0.0;
  if (out.min) out.min[c] = canonical_nan();
  if (out.max) out.max[c] = canonical_nan();
  if (out.mean) out.mean[c] = canonical_nan();
  if (out.variance) out.variance[c] = canonical_nan();
}

// ---- the atomic path ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void raster_atomic_kernel(Pos pos, uint64_t n, Input in, Grid g, unsigned long long* min_keys, unsigned long long* max_keys,
                                                               uint32_t* counts, unsigned long long* members) {
  const uint64_t first = (uint64_t)blockIdx.x * kPpb;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPpb / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    uint32_t cell;
    double v;
    if (!member_cell(pos, i, in, g, cell, v)) continue;
    mine += 1;
    const unsigned long long key = ordered(v);  // a finite value: neither all ones nor zero, the two empty marks
    if (min_keys && key < __hip_atomic_load(min_keys + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(min_keys + cell, key);
    if (max_keys && key > __hip_atomic_load(max_keys + cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_keys + cell, key);
    if (counts) atomicAdd(counts + cell, 1u);
  }
  block_count(mine, members);
}

__global__ __launch_bounds__(kBlock) void raster_atomic_decode_kernel(const unsigned long long* __restrict__ min_keys, const unsigned long long* __restrict__ max_keys,
                                                                      const uint32_t* __restrict__ counts, uint64_t n_cells, Planes out) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cells) return;
  if (out.count) out.count[c] = (double)counts[c];
  if (out.min) {
    const unsigned long long key = min_keys[c];
    out.min[c] = key == ~0ull ? canonical_nan() : decode_ordered(key);
  }
  if (out.max) {
    const unsigned long long key = max_keys[c];
    out.max[c] = key == 0ull ? canonical_nan() : decode_ordered(key);
  }
}

// ---- the sorted path: keys, directory, gather ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void raster_key_kernel(Pos pos, uint64_t n, Input in, Grid g, uint32_t nonmember_key, uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t cell;
  double v;
  keys[i] = member_cell(pos, i, in, g, cell, v) ? cell : nonmember_key;
}

// The heads of every dense directory (pstk::directory_heads).  A key's group: (key >> bx) * cols + the low bx bits -- a label or a row-major
// cell is its own group (bx = 0, cols = 1), a packed (cy << bx) | cx its cell cy * cols + cx.
__global__ __launch_bounds__(kBlock) void directory_heads_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t bx, uint32_t cols, uint32_t groups,
                                                                 uint32_t* __restrict__ dir) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  const uint32_t key = keys[s];
  const uint32_t group = (key >> bx) * cols + (key & ((1u << bx) - 1u));
  const bool is_member = group < groups;  // (every other key is a power of two whose group is not below `groups`)
  const bool head = s == 0 || key != keys[s - 1];
  if (is_member) {
    if (head) dir[group] = s;
    if (s == n - 1) dir[groups] = n;  // every entry is a member
  } else if (head) {
    dir[groups] = s;  // the first entry that is not one
  }
}

__global__ __launch_bounds__(kBlock) void raster_gather_kernel(Pos pos, Input in, const uint32_t* __restrict__ order, const uint32_t* __restrict__ dir, uint32_t n_cells,
                                                               double* __restrict__ sorted_values) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= dir[n_cells]) return;
  const uint32_t i = order[s];
  sorted_values[s] = in.values ? in.values[i] : load_un<double>(pos.base + (uint64_t)i * pos.stride + 16);
}

// ---- the sorted path: the reduction ---------------------------------------------------------------------------------------------------------------
// A cell of at most one chunk: one lane, all planes.
__global__ __launch_bounds__(kBlock) void raster_reduce_kernel(const double* __restrict__ vals, const uint32_t* __restrict__ dir, uint32_t n_cells, uint32_t stats,
                                                               Planes out, uint32_t* __restrict__ heavy_list, uint32_t* heavy_count) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cells) return;
  const uint32_t first = dir[c], m = dir[c + 1] - first;
  if (out.count) out.count[c] = (double)m;
  if (m > kChunk) {  // the heavy-cell pass writes its other planes
    heavy_list[atomicAdd(heavy_count, 1u)] = c;
    return;
  }
  double mn = canonical_nan(), mx = canonical_nan(), mean = canonical_nan(), var = canonical_nan();
  if (m) {
    const double* p = vals + first;
    double sum = p[0];
    unsigned long long kmin = ordered(sum), kmax = kmin;
    for (uint32_t t = 1; t < m; ++t) {
      const double v = p[t];
      const unsigned long long key = ordered(v);
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
      sum = sum + v;
    }
    mn = decode_ordered(kmin);
    mx = decode_ordered(kmax);
    mean = sum / (double)m;
    if (stats & pstk::RS_VARIANCE) {
      double d = p[0] - mean;
      double ss = d * d;
      for (uint32_t t = 1; t < m; ++t) {
        d = p[t] - mean;
        ss = ss + d * d;
      }
      var = ss / (double)m;
    }
  }
  if (out.min) out.min[c] = mn;
  if (out.max) out.max[c] = mx;
  if (out.mean) out.mean[c] = mean;
  if (out.variance) out.variance[c] = var;
}

// A heavy cell's chunk partials.  Where they live: a cell whose segment starts at sorted position `first` owns the slots from
// 2 * (first / 256).  It has k = ceil(m / 256) <= 2 * floor(m / 256) chunks (m > 256), and the next cell starts at first + m or later, whose
// slots begin at 2 * floor((first + m) / 256) >= 2 * floor(first / 256) + 2 * floor(m / 256): the ranges of two cells never overlap, and all
// of them end below 2 * (n / 256 + 1).  The partials of SS take a second region of that size.
__device__ __forceinline__ size_t partial_slots(uint64_t n) { return 2 * (size_t)(n / kChunk + 1); }

// thread t: chunks t, t + 256, ... of the segment p[0, m), each summed left to right from its first element; kSquares: of (v - mean)^2
template <bool kSquares>
__device__ __forceinline__ void chunk_partials(const double* __restrict__ p, uint32_t m, double mean, double* __restrict__ partials, unsigned long long& kmin,
                                               unsigned long long& kmax) {
  const uint32_t chunks = (m + kChunk - 1) / kChunk;
#pragma unroll 1
  for (uint32_t j = threadIdx.x; j < chunks; j += kBlock) {
    const uint32_t b = j * kChunk, e = b + kChunk < m ? b + kChunk : m;
    double acc;
    if (kSquares) {
      const double d = p[b] - mean;
      acc = d * d;
    } else {
      acc = p[b];
      const unsigned long long key = ordered(acc);
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
    }
#pragma unroll 8
    for (uint32_t t = b + 1; t < e; ++t) {
      const double v = p[t];
      if (kSquares) {
        const double d = v - mean;
        acc = acc + d * d;
      } else {
        const unsigned long long key = ordered(v);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
        acc = acc + v;
      }
    }
    partials[j] = acc;
  }
}

__device__ __forceinline__ double fold_partials(const double* partials, uint32_t chunks) {
  double s = partials[0];
  for (uint32_t j = 1; j < chunks; ++j) s = s + partials[j];
  return s;
}

__global__ __launch_bounds__(kBlock) void raster_heavy_kernel(const double* __restrict__ vals, const uint32_t* __restrict__ dir, uint32_t n, uint32_t stats, Planes out,
                                                              const uint32_t* __restrict__ heavy_list, const uint32_t* __restrict__ heavy_count, double* partials) {
  __shared__ unsigned long long s_min[kBlock / 64], s_max[kBlock / 64];
  __shared__ double s_mean;
  const uint32_t heavy = *heavy_count;
#pragma unroll 1
  for (uint32_t h = blockIdx.x; h < heavy; h += gridDim.x) {  // (the same trip count in every thread: the barriers below are uniform)
    const uint32_t c = heavy_list[h];
    const uint32_t first = dir[c], m = dir[c + 1] - first;
    const uint32_t chunks = (m + kChunk - 1) / kChunk;
    const double* p = vals + first;
    double* mine = partials + 2 * (size_t)(first / kChunk);
    unsigned long long kmin = ~0ull, kmax = 0ull;
    chunk_partials<false>(p, m, 0.0, mine, kmin, kmax);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long a = shfl_xor_any(kmin, off), b = shfl_xor_any(kmax, off);
      kmin = a < kmin ? a : kmin;
      kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0) { s_min[threadIdx.x >> 6] = kmin; s_max[threadIdx.x >> 6] = kmax; }
    __syncthreads();  // the partials (global memory, this workgroup's own) and the waves' extremes
    if (threadIdx.x == 0) {
#pragma unroll
      for (uint32_t w = 1; w < kBlock / 64; ++w) {
        kmin = s_min[w] < kmin ? s_min[w] : kmin;
        kmax = s_max[w] > kmax ? s_max[w] : kmax;
      }
      const double mean = fold_partials(mine, chunks) / (double)m;
      s_mean = mean;
      if (out.min) out.min[c] = decode_ordered(kmin);
      if (out.max) out.max[c] = decode_ordered(kmax);
      if (out.mean) out.mean[c] = mean;
    }
    __syncthreads();
    if (stats & pstk::RS_VARIANCE) {
      double* squares = mine + partial_slots(n);
      chunk_partials<true>(p, m, s_mean, squares, kmin, kmax);
      __syncthreads();
      if (threadIdx.x == 0) out.variance[c] = fold_partials(squares, chunks) / (double)m;
    }
    __syncthreads();  // s_min, s_max and s_mean are written again by the next cell
  }
}

// ---- the fill ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void raster_fill_kernel(const double* __restrict__ in, double* __restrict__ out, uint32_t cols, uint32_t rows, uint32_t h,
                                                             uint32_t tiles_x) {
  __shared__ double tile[kFillDoubles];
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int64_t c0 = (int64_t)tx * kTc, r0 = (int64_t)ty * kTr;
  const uint32_t ext_c = kTc + 2 * h, ext_r = kTr + 2 * h;  // ext_c * ext_r <= kFillDoubles: h <= kFh (the launcher)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t lr = wave; lr < ext_r; lr += kBlock / 64) {
    const int64_t r = r0 - (int64_t)h + lr;
    for (uint32_t lc = lane; lc < ext_c; lc += 64) {
      const int64_t c = c0 - (int64_t)h + lc;
      double v = canonical_nan();  // outside the raster: never visited
      if (r >= 0 && r < (int64_t)rows && c >= 0 && c < (int64_t)cols) v = in[(size_t)r * cols + (size_t)c];
      tile[lr * ext_c + lc] = v;
    }
  }
  __syncthreads();
  const int64_t c = c0 + lane;
  if (c >= (int64_t)cols) return;
  const int ih = (int)h;
#pragma unroll 1
  for (uint32_t row = wave; row < kTr; row += kBlock / 64) {
    const int64_t r = r0 + row;
    if (r >= (int64_t)rows) break;
    const double* centre = tile + (row + h) * ext_c + (lane + h);
    double v = *centre;
    if (!finite(v)) {
      double num = 0.0, den = 0.0;
      bool any = false;
      for (int dr = -ih; dr <= ih; ++dr) {
        const double* p = centre + dr * (int)ext_c;
        for (int dc = -ih; dc <= ih; ++dc) {
          const double u = p[dc];
          if (!finite(u)) continue;  // (the cell itself is one of these: dr * dr + dc * dc is never zero below)
          const double w = 1.0 / (double)(dr * dr + dc * dc);
          num = any ? num + w * u : w * u;
          den = any ? den + w : w;
          any = true;
        }
      }
      v = any ? num / den : canonical_nan();
    }
    out[(size_t)r * cols + (size_t)c] = v;
  }
}

}  // namespace

namespace pstk {

bool raster_fill_empty(const RasterPlanes& out, uint64_t n_cells, hipStream_t stream) {
  hipLaunchKernelGGL(raster_fill_empty_kernel, dim3(blocks_of(n_cells, kBlock)), dim3(kBlock), 0, stream, out, n_cells);
  return launched();
}

bool raster_atomic(const Positions& pos, const RasterInput& in, const PmfGrid& g, unsigned long long* min_keys, unsigned long long* max_keys, uint32_t* counts,
                   unsigned long long* members, hipStream_t stream) {
  hipLaunchKernelGGL(raster_atomic_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, in, g, min_keys, max_keys, counts, members);
  return launched();
}

bool raster_atomic_decode(const unsigned long long* min_keys, const unsigned long long* max_keys, const uint32_t* counts, uint64_t n_cells, const RasterPlanes& out,
                          hipStream_t stream) {
  hipLaunchKernelGGL(raster_atomic_decode_kernel, dim3(blocks_of(n_cells, kBlock)), dim3(kBlock), 0, stream, min_keys, max_keys, counts, n_cells, out);
  return launched();
}

bool raster_keys(const Positions& pos, const RasterInput& in, const PmfGrid& g, uint32_t nonmember_key, uint32_t* keys, hipStream_t stream) {
  hipLaunchKernelGGL(raster_key_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, in, g, nonmember_key, keys);
  return launched();
}

bool directory_heads(const uint32_t* sorted_keys, uint32_t n, uint32_t bx, uint32_t cols, uint32_t groups, uint32_t* dir, hipStream_t stream) {
  hipLaunchKernelGGL(directory_heads_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, sorted_keys, n, bx, cols, groups, dir);
  return launched();
}

bool raster_gather(const Positions& pos, const RasterInput& in, const uint32_t* order, const uint32_t* dir, uint32_t n_cells, double* sorted_values, hipStream_t stream) {
  hipLaunchKernelGGL(raster_gather_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), in, order, dir, n_cells, sorted_values);
  return launched();
}

size_t raster_partials_bytes(uint64_t n) { return 2 * 2 * (size_t)(n / kChunk + 1) * sizeof(double); }

bool raster_reduce(const double* sorted_values, const uint32_t* dir, uint32_t n_cells, uint32_t stats, const RasterPlanes& out, uint32_t* heavy_list, uint32_t* heavy_count,
                   hipStream_t stream) {
  hipLaunchKernelGGL(raster_reduce_kernel, dim3(blocks_of(n_cells, kBlock)), dim3(kBlock), 0, stream, sorted_values, dir, n_cells, stats, out, heavy_list, heavy_count);
  return launched();
}

bool raster_reduce_heavy(const double* sorted_values, const uint32_t* dir, uint32_t n, uint32_t n_cells, uint32_t stats, const RasterPlanes& out, const uint32_t* heavy_list,
                         const uint32_t* heavy_count, double* partials, hipStream_t stream) {
  const uint64_t most = std::min<uint64_t>(n / (kChunk + 1), n_cells);  // cells of more than one chunk there can be
  if (most == 0) return true;
  hipLaunchKernelGGL(raster_heavy_kernel, dim3((unsigned)std::min<uint64_t>(most, kRasterHeavyBlocks)), dim3(kBlock), 0, stream, sorted_values, dir, n, stats, out,
                     heavy_list, heavy_count, partials);
  return launched();
}

bool raster_grid_fill(const double* in, double* out, uint32_t cols, uint32_t rows, uint32_t h, hipStream_t stream) {
  if (h > kFh || cols == 0 || rows == 0 || (uint64_t)cols * rows > (1ull << 28)) return false;  // (the tile and the index arithmetic rely on it)
  const uint32_t tiles_x = (cols + kTc - 1) / kTc, tiles_y = (rows + kTr - 1) / kTr;
  hipLaunchKernelGGL(raster_fill_kernel, dim3(tiles_x * tiles_y), dim3(kBlock), 0, stream, in, out, cols, rows, h, tiles_x);
  return launched();
}

}  // namespace pstk
