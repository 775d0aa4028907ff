// Ground classification by the progressive morphological filter (Zhang et al. 2003; include/pasture_amd.h, "Ground classification").
//
// Pipeline (pmf_api.cpp drives it; the host reads one small record in between):
//   bounds    clusters.hip's AABB of the FINITE points and their number
//   raster    Z_0[cell] = min z of the cell's finite points: one pass over the positions, a FILTERED 64-bit atomicMin per point
//   opening   per window k: E = erode(Z_k, h_k), D = dilate(E, h_k), L = min(L, D + th_k), Z_{k+1} = D.  Every erode / dilate is separable:
//             a pass along the columns, then a pass along the rows, each an LDS tile with a halo of h cells on both sides of its axis
//   classify  one pass over the positions: ground iff finite and z <= L[cell]; one mask byte per point, one integer atomic per workgroup
// Everything is min / max of f64 values and one f64 addition per cell and window: no result depends on the order of evaluation.
//
// A pass handles h <= kPmfMaxHalfWidth (kernels.hpp: the LDS budget).  A larger h runs as successive passes whose half-widths add up to h:
// min over |d| <= h1 of the min over |e| <= h2 is the min over |d + e| <= h1 + h2, because every in-raster target within h1 + h2 of a cell is
// reached through an in-raster intermediate cell (the interval between the two is inside the raster) -- so clipping changes nothing.  The same
// holds for the max over the entries below +inf: "ignored" is the identity of that max, and a pass writes +inf exactly where it found none.
//
// The tile.  A workgroup writes kPmfTileRows x kPmfTileCols cells; lane l of every wave owns column l of the tile in BOTH passes, so global
// loads and stores run along the raster's columns (one row of 64 doubles = 512 contiguous bytes per wave instruction), and every LDS access
// of a wave is 64 consecutive doubles of one tile row: ds_read_b64 / ds_write_b64 over consecutive addresses, each 32-lane half on one 256-byte
// bank row -- no bank conflicts in the column pass, the row pass or the halo load, whatever h makes the row length.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPpb = pstk::kPmfPointsPerBlock;
constexpr uint32_t kTc = pstk::kPmfTileCols, kTr = pstk::kPmfTileRows, kH = pstk::kPmfMaxHalfWidth;
constexpr uint32_t kTileDoubles = (kTr + 2 * kH) * kTc;  // the column pass's tile; the row pass's is kTr x (kTc + 2 H), never larger
static_assert(kTc == 64 && kBlock == 256 && kTr % (kBlock / 64) == 0, "one wave per tile row, lane = column");
static_assert(kTr * (kTc + 2 * kH) <= kTileDoubles && kTileDoubles * sizeof(double) <= 48 * 1024, "the LDS budget kPmfMaxHalfWidth is chosen from");
static_assert(kPpb % kBlock == 0, "whole points per lane");

using Grid = pstk::PmfGrid;

// THE cell of a point: the raster pass and the classification pass both call this, and pmf_api.cpp sizes the raster from the largest x and y
// by the same expression (the subtraction and the division are monotone, so no point lands beyond it; the clamp is never taken)
__device__ __forceinline__ void pmf_cell(const Grid& g, double x, double y, uint32_t& row, uint32_t& col) {
  const uint32_t c = (uint32_t)((x - g.x0) / g.cell), r = (uint32_t)((y - g.y0) / g.cell);  // 0 <= quotient < 2^28: the conversion truncates
  col = c < g.cols ? c : g.cols - 1;
  row = r < g.rows ? r : g.rows - 1;
}

// ---- min-z raster ---------------------------------------------------------------------------------------------------------------------------
// Per finite point: a plain load of the cell's key, and the 64-bit atomicMin only when the point's key is smaller.  The skip is safe because a
// cell's key only ever DECREASES: whatever (possibly stale) value the load returns is >= the value the cell holds now and will hold later, so
// "my key is not below what I read" implies "my key is not below the final minimum" -- and the point could not have changed it.  A stale read
// can only make a point issue an atomic it did not need; it can never lose a minimum.
__global__ __launch_bounds__(kBlock) void pmf_raster_kernel(Pos pos, uint64_t n, Grid g, unsigned long long* cells) {
  const uint64_t first = (uint64_t)blockIdx.x * kPpb;
#pragma unroll
  for (uint32_t j = 0; j < kPpb / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    double x, y, z;
    load_point(pos, i, x, y, z);
    if (!(finite(x) && finite(y) && finite(z))) continue;
    uint32_t row, col;
    pmf_cell(g, x, y, row, col);
    unsigned long long* cell = cells + ((size_t)row * g.cols + col);
    const unsigned long long key = ordered(z);
    if (key < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(cell, key);
  }
}

// ---- grid morphology ------------------------------------------------------------------------------------------------------------------------
// kAxis 0: along the columns (the tile is kTr rows of kTc + 2 h cells); kAxis 1: along the rows (kTr + 2 h rows of kTc cells).
// Cells outside the raster and, for the max, entries that are not below +inf load as the identity of the fold.
template <bool kMax, int kAxis>
__global__ __launch_bounds__(kBlock) void pmf_morphology_kernel(const void* __restrict__ in, int in_is_keys, double* __restrict__ out, uint32_t cols, uint32_t rows,
                                                                uint32_t h, uint32_t tiles_x, double* __restrict__ L, int fold, double th) {
  __shared__ double tile[kTileDoubles];
  constexpr double ident = kMax ? -kInf : kInf;
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int64_t c0 = (int64_t)tx * kTc, r0 = (int64_t)ty * kTr;
  const uint32_t ext_c = kTc + (kAxis == 0 ? 2 * h : 0), ext_r = kTr + (kAxis == 1 ? 2 * h : 0);  // ext_c * ext_r <= kTileDoubles: h <= kH (the launcher)
  const int64_t lc0 = c0 - (kAxis == 0 ? (int64_t)h : 0), lr0 = r0 - (kAxis == 1 ? (int64_t)h : 0);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t lr = wave; lr < ext_r; lr += kBlock / 64) {
    const int64_t r = lr0 + lr;
    for (uint32_t lc = lane; lc < ext_c; lc += 64) {
      const int64_t c = lc0 + lc;
      double v = ident;
      if (r >= 0 && r < (int64_t)rows && c >= 0 && c < (int64_t)cols) {
        const size_t at = (size_t)r * cols + (size_t)c;
        if (in_is_keys) {
          const unsigned long long key = ((const unsigned long long*)in)[at];
          v = key == ~0ull ? kInf : decode_ordered(key);
        } else {
          v = ((const double*)in)[at];
        }
        if (kMax) v = v < kInf ? v : -kInf;  // (a NaN is ignored like +inf; the min skips it by itself)
      }
      tile[lr * ext_c + lc] = v;
    }
  }
  __syncthreads();
  const int64_t c = c0 + lane;
  if (c >= (int64_t)cols) return;
  const uint32_t step = kAxis == 0 ? 1 : ext_c;
#pragma unroll 1
  for (uint32_t row = wave; row < kTr; row += kBlock / 64) {
    const int64_t r = r0 + row;
    if (r >= (int64_t)rows) break;
    const double* p = tile + row * ext_c + lane;  // the window's first entry: h cells before the output cell along the axis
    double acc = ident;
    for (uint32_t d = 0; d <= 2 * h; ++d) acc = kMax ? fold_max(acc, p[d * step]) : fold_min(acc, p[d * step]);
    if (kMax) acc = acc > -kInf ? acc : kInf;  // none below +inf
    const size_t at = (size_t)r * cols + (size_t)c;
    out[at] = acc;
    if (fold == 1) L[at] = acc + th;
    else if (fold == 2) L[at] = fold_min(L[at], acc + th);
  }
}

__global__ __launch_bounds__(kBlock) void pmf_decode_kernel(unsigned long long* cells, uint64_t n_cells) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_cells) return;
  const unsigned long long key = cells[i];
  ((double*)cells)[i] = key == ~0ull ? kInf : decode_ordered(key);
}

// ---- classification -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pmf_classify_kernel(Pos pos, uint64_t n, Grid g, const double* __restrict__ L, uint8_t* __restrict__ mask,
                                                              unsigned long long* count) {
  __shared__ uint32_t wave_count[kBlock / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kPpb;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPpb / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    double x, y, z;
    load_point(pos, i, x, y, z);
    bool ground = false;
    if (finite(x) && finite(y) && finite(z)) {
      uint32_t row, col;
      pmf_cell(g, x, y, row, col);
      ground = z <= L[(size_t)row * g.cols + col];
    }
    mask[i] = ground ? 1 : 0;
    mine += ground ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine += shfl_xor_any(mine, off);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) total += wave_count[w];
    if (total) atomicAdd(count, total);
  }
}

__global__ __launch_bounds__(kBlock) void set_u8_where_kernel(gptr_t base, uint64_t stride, uint64_t n, const uint8_t* __restrict__ mask, uint8_t value) {
  const uint64_t first = (uint64_t)blockIdx.x * kPpb;
#pragma unroll
  for (uint32_t j = 0; j < kPpb / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i < n && mask[i]) *(base + i * stride) = value;
  }
}

__global__ __launch_bounds__(kBlock) void finite_mask_kernel(Pos pos, uint64_t n, uint8_t* __restrict__ mask) {
  const uint64_t first = (uint64_t)blockIdx.x * kPpb;
#pragma unroll
  for (uint32_t j = 0; j < kPpb / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    double x, y, z;
    load_point(pos, i, x, y, z);
    mask[i] = finite(x) && finite(y) && finite(z) ? 1 : 0;
  }
}

template <bool kMax, int kAxis>
void launch_pass(const void* in, bool in_is_keys, double* out, uint32_t cols, uint32_t rows, uint32_t h, double* L, int fold, double th, hipStream_t stream) {
  const uint32_t tiles_x = (cols + kTc - 1) / kTc, tiles_y = (rows + kTr - 1) / kTr;  // cols * rows <= 2^28: at most 2^23 tiles
  hipLaunchKernelGGL((pmf_morphology_kernel<kMax, kAxis>), dim3(tiles_x * tiles_y), dim3(kBlock), 0, stream, in, in_is_keys ? 1 : 0, out, cols, rows, h, tiles_x, L, fold,
                     th);
}

}  // namespace

namespace pstk {

bool pmf_raster(const Positions& pos, const PmfGrid& g, unsigned long long* cells, hipStream_t stream) {
  hipLaunchKernelGGL(pmf_raster_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, g, cells);
  return launched();
}

bool pmf_morphology_pass(const void* in, bool in_is_keys, double* out, uint32_t cols, uint32_t rows, uint32_t h, bool dilate, int axis, double* L, int fold, double th,
                         hipStream_t stream) {
  if (h > kH || cols == 0 || rows == 0 || (uint64_t)cols * rows > (1ull << 28) || (fold && !L)) return false;  // (the tile and the index arithmetic rely on it)
  if (dilate) {
    if (axis == 0) launch_pass<true, 0>(in, in_is_keys, out, cols, rows, h, L, fold, th, stream);
    else launch_pass<true, 1>(in, in_is_keys, out, cols, rows, h, L, fold, th, stream);
  } else {
    if (axis == 0) launch_pass<false, 0>(in, in_is_keys, out, cols, rows, h, L, fold, th, stream);
    else launch_pass<false, 1>(in, in_is_keys, out, cols, rows, h, L, fold, th, stream);
  }
  return launched();
}

bool pmf_decode_keys(unsigned long long* cells, uint64_t n_cells, hipStream_t stream) {
  hipLaunchKernelGGL(pmf_decode_kernel, dim3(blocks_of(n_cells, kBlock)), dim3(kBlock), 0, stream, cells, n_cells);
  return launched();
}

bool pmf_classify(const Positions& pos, const PmfGrid& g, const double* L, uint8_t* mask, unsigned long long* count, hipStream_t stream) {
  hipLaunchKernelGGL(pmf_classify_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, g, L, mask, count);
  return launched();
}

bool finite_mask(const Positions& pos, uint8_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(finite_mask_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, mask);
  return launched();
}

bool set_u8_where(uint64_t addr, uint64_t stride, uint64_t n, const uint8_t* mask, uint8_t value, hipStream_t stream) {
  hipLaunchKernelGGL(set_u8_where_kernel, dim3(blocks_of(n, kPpb)), dim3(kBlock), 0, stream, (gptr_t)addr, stride, n, mask, value);
  return launched();
}

}  // namespace pstk
