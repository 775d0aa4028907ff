// Height above ground from the k nearest ground points in the XY plane, inverse-squared-distance weighted (include/pasture_amd.h, "Height
// above ground").
//
// Definitions.  G = the points of the ground buffer with three finite components and a non-zero mask byte.  For a finite query q,
// d2(q, p) = dx*dx + dy*dy with dx = p.x - q.x, dy = p.y - q.y; its neighbours are the at most k members of G with the lexicographically
// smallest (d2, ground-buffer index) among those with d2 <= m2.  w_i = 1.0 / d2_i; an exact hit (w_0 not below +inf) gives zg = z_0, else
// num = w_0*z_0 (+ w_i*z_i in order), den = w_0 (+ w_i in order), zg = num / den.  Every operation a separately rounded f64 operation.
//
// The index is rebuilt by every call (hag_api.cpp): G sorted by cell key, x, y, z in that order as three f64 arrays next to the buffer index
// of every sorted position, and the dense directory -- keys, directory and the ring walk with its exactness argument are
// dense_grid_device.hpp's, with G as the members and last.d2 as the bound.
//
// The search, one lane per query, one wave per workgroup, queries in cell order (clamped into the AABB and keyed like a ground point, then
// sorted: the lanes of a wave are neighbours and read the same candidates).  The lane keeps its k best (d2, index, sorted position) as a
// sorted list in LDS, laid out [slot][lane]: a wave's access to one slot is 64 consecutive words, and a lane's column sits in the same
// banks whatever the slot, so lanes at different slots do not conflict either.  Every slot starts at (m2, 0xFFFFFFFF) and a candidate enters
// when it is lexicographically below the LAST slot: the bound, "fewer than k so far" and the tie rule are that one compare, and the order in
// which candidates arrive cannot matter.  The last slot's pair is mirrored in two registers, so a candidate that does not enter costs no LDS
// access.  The result depends on the two clouds, the mask, k and max_distance alone.
#include "dense_grid_device.hpp"

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

__device__ __forceinline__ bool finite3(double x, double y, double z) { return finite(x) && finite(y) && finite(z); }

// ---- masked 2-D bounds and count of G ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hag_bounds_partial_kernel(Pos pos, uint64_t n, const uint8_t* __restrict__ mask, Bounds* __restrict__ partials) {
  __shared__ double sv[4 * 2 * 2];
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
  __shared__ double sv[4 * 2 * 2];
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

// ---- keys ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void hag_ground_key_kernel(Pos pos, uint64_t n, const uint8_t* __restrict__ mask, Grid g, uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t key = no_member_key(g);  // not in G
  if (!mask || mask[i]) {
    double x, y, z;
    load_point(pos, i, x, y, z);
    if (finite3(x, y, z)) key = member_key(x, y, g);
  }
  keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void hag_query_key_kernel(Pos pos, uint64_t n, Grid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  load_point(pos, i, x, y, z);
  keys[i] = finite3(x, y, z) ? query_key(x, y, g) : no_member_key(g);  // (not finite: behind every finite query)
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
    double zg = kNaN, qz = kNaN;
    if (is_member_key(key, g)) {  // a finite query
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
      uint32_t cx, cy;
      cell_of_key(key, g, cx, cy);
      walk_rings(g, dir, cx, cy, [&](uint32_t first, uint32_t last) { scan(xs, ys, gidx, first, last, qx, qy, l); }, [&] { return l.last_d2; });
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
