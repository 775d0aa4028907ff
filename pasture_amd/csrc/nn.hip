// Nearest neighbours between two clouds and the sums of an ICP step (include/pasture_amd.h, "Nearest neighbours between two clouds, ICP").
//
// Definitions.  A query q is first sent through the optional transform, x' = ((r00*x + r01*y) + r02*z) + t0 (y', z' alike); its match is the finite
// target p with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = p.x - q'.x, among those with d2 <= m2 = max_distance * max_distance, equal d2
// going to the lower target buffer index; every operation a separately rounded f64 operation.  No match: index 0xFFFFFFFF, distance +inf.
//
// The index (nn_api.cpp builds it) is the cluster grid: the finite targets sorted by cell key, key = (cz << (bx + by)) | (cy << bx) | cx with
// cell = trunc((v - min) / edge) per axis over the finite targets' AABB, their positions in that order as three f64 arrays, and the buffer
// index of every sorted position.
//
// The search, one lane per query, queries in cell order.  The transformed query is clamped into the AABB, c = clamp(q'), keyed by c's cell
// like a target, and (key, query index) is sorted: the lanes of a wave are neighbours, walk the same rows and read the same candidates.  A
// lane visits the cells at Chebyshev cell distance 1 and less from c's cell (ring 0 and ring 1 in one pass), then ring 2, 3, ..., clipped to
// the grid.  In the key order every (y, z) row of cells is contiguous: a row on a ring's face is one key range [x - r, x + r], a row inside
// the ring is its two end cells, each found by binary searches of the sorted keys.  The best (d2, buffer index) pair so far is replaced by a
// candidate that is lexicographically smaller; it starts at (m2, 0xFFFFFFFF), so the bound and "no match" need no case of their own, and
// the order in which candidates arrive cannot matter.
//
// When the walk may stop: after ring r as soon as best_d2 <= (r * edge_stop)^2, edge_stop = edge * (1 - 2^-20).  The argument:
//   clamping   every target lies in the AABB and clamping moves a coordinate of q' onto the nearest point of [min, max] exactly (a min / max
//              of two doubles does not round), so per axis |p - q'| >= |p - c| as real numbers, for every target p.
//   cells      a target p that rings 0 .. r have not visited is more than r cells from c's cell on some axis: its cell numbers
//              trunc(fl(fl(p - min) / edge)) and trunc(fl(fl(c - min) / edge)) differ by r + 1 or more there, so the computed quotients differ by
//              MORE than r.  Each carries two roundings of a value below 2^21, an absolute error below 2^-31: the exact quotients differ
//              by more than r - 2^-30, that is |p - c| > (r - 2^-30) * edge >= r * edge * (1 - 2^-30) on that axis (r >= 1).
//   margin     hence |p - q'| > r * edge * (1 - 2^-30) on that axis, and the computed d2 -- a rounded difference, its rounded square, two
//              rounded sums of non-negative terms, each within 2^-53 relative and monotonic -- is at least (r * edge)^2 * (1 - 2^-28).
//              (r * edge_stop)^2 as the kernel computes it is at most (r * edge)^2 * (1 - 2^-20)^2 * (1 + 2^-51) < (r * edge)^2 * (1 - 2^-20).
//              So d2(p) > (r * edge_stop)^2 >= best_d2 STRICTLY: an unvisited point can neither win nor tie, and the tie rule is decided
//              among visited points alone.  The margin 2^-20 is the cluster grid's; it is some 2^8 times what the roundings need.
//   a dim of 1 all cell numbers of that axis are 0 and no ring leaves it: the axis never is "the axis more than r cells away", the bound
//              rests on the others.  When r reaches the largest cell distance to any face of the grid every cell has been visited and the
//              walk ends whatever best_d2 is (an unbounded search of a query with no match never happens with one finite target).
//   the cell of the largest coordinate is dim - 1 by the expression the host sized dim with, so the clamp of a cell number is never taken
//   for a target, and c lies in [min, max], so it is not for a query either.
// The result depends on the two clouds, the transform and max_distance alone: the grid decides which points are LOOKED AT, never which
// one wins.  A query far outside a large target visits ring after ring until its bound holds -- up to the whole grid.  That is accepted:
// scans that are aligned well enough to be matched do not do it, and max_distance bounds the walk to ceil(max_distance / edge_stop) rings.
//
// The ICP sums have a fixed shape, like outliers.hip: block b of the partial kernels owns source points [b * kNnReducePoints, ...), a thread
// adds its four points (stride kBlock) in order, the wave folds in a fixed xor tree, the four waves' sums are added in wave order; ONE
// workgroup then adds the block partials, thread t the contiguous run [t * c, (t + 1) * c) in block order, then the same tree.  No
// floating-point atomics: two calls give the same bits.
//
// The point-to-plane step (nn_plane_*_kernel) has the same two passes over the pairs whose target normal is finite and not zero: cq and
// sum d2 first, then with w = q' - cq, a = w x n, r = (p - q') . n, j = (a, n) the 21 + 6 + 2 sums A = sum j j^T (upper triangle), g = sum j r,
// sum r^2, sum |w|^2.  The normals are the index's, gathered into its sorted order by nn_gather_normals_kernel and used as given.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kQ = pstk::kNnQueriesPerBlock;
constexpr uint32_t kRP = pstk::kNnReducePoints;
constexpr uint32_t kRB = pstk::kNnReduceBlock;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kQ == kBlock && kRB == kBlock && kRP % kBlock == 0, "one lane per query; the reduction kernels are written for one kBlock workgroup");

using Grid = pstk::NnGrid;
using Xform = pstk::NnTransform;

__device__ __forceinline__ void apply(const Xform& t, double& x, double& y, double& z) {
  if (!t.on) return;
  const double a = ((t.m[0] * x + t.m[1] * y) + t.m[2] * z) + t.m[3];
  const double b = ((t.m[4] * x + t.m[5] * y) + t.m[6] * z) + t.m[7];
  const double c = ((t.m[8] * x + t.m[9] * y) + t.m[10] * z) + t.m[11];
  x = a; y = b; z = c;
}

__device__ __forceinline__ uint32_t cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;  // 0 <= q < 2^21: the conversion truncates
  return c < dim ? c : dim - 1;    // (never taken, see above)
}
__device__ __forceinline__ double clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first position in keys[lo, hi) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const unsigned long long* __restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long k) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- index build ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nn_gather_kernel(Pos pos, const uint32_t* __restrict__ order, uint32_t nf, double* __restrict__ xs, double* __restrict__ ys,
                                                           double* __restrict__ zs) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= nf) return;
  double x, y, z;
  load_point(pos, order[s], x, y, z);
  xs[s] = x; ys[s] = y; zs[s] = z;
}

// occupied cells = positions of the sorted keys whose key differs from the one before
__global__ __launch_bounds__(kBlock) void nn_count_cells_kernel(const unsigned long long* __restrict__ keys, uint32_t nf, unsigned long long* __restrict__ count) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  const bool head = s < nf && (s == 0 || keys[s] != keys[s - 1]);
  const unsigned long long c = (unsigned long long)__popcll(__ballot(head));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// ---- query keys -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nn_query_key_kernel(Pos pos, uint64_t n, Xform t, Grid g, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  load_point(pos, i, x, y, z);
  apply(t, x, y, z);
  unsigned long long key = ~0ull;  // not finite: behind every finite query
  if (finite(x) && finite(y) && finite(z)) {
    const unsigned long long cx = cell_of(clamp(x, g.min[0], g.max[0]), g.min[0], g.edge, g.dim[0]);
    const unsigned long long cy = cell_of(clamp(y, g.min[1], g.max[1]), g.min[1], g.edge, g.dim[1]);
    const unsigned long long cz = cell_of(clamp(z, g.min[2], g.max[2]), g.min[2], g.edge, g.dim[2]);
    key = (cz << (g.bits[0] + g.bits[1])) | (cy << g.bits[0]) | cx;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// ---- the search -------------------------------------------------------------------------------------------------------------------------------
struct Best { double d2; uint32_t idx, at; };

__device__ __forceinline__ void scan(const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ zs, const uint32_t* __restrict__ tidx,
                                     uint32_t first, uint32_t last, double qx, double qy, double qz, Best& b) {
  for (uint32_t c = first; c < last; ++c) {
    const double dx = xs[c] - qx, dy = ys[c] - qy, dz = zs[c] - qz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 <= b.d2) {
      const uint32_t j = tidx[c];
      if (d2 < b.d2 || j < b.idx) { b.d2 = d2; b.idx = j; b.at = c; }
    }
  }
}

// order == nullptr: query s is point s (no finite target: nothing to walk, every query is unmatched)
__global__ __launch_bounds__(kBlock) void nn_search_kernel(Pos pos, uint32_t nq, Xform t, Grid g, double m2, const unsigned long long* __restrict__ qkeys,
                                                           const uint32_t* __restrict__ order, const unsigned long long* __restrict__ keys,
                                                           const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ zs,
                                                           const uint32_t* __restrict__ tidx, uint32_t nf, uint32_t* __restrict__ out_idx,
                                                           double* __restrict__ out_dist, uint32_t* __restrict__ out_at) {
  const uint32_t s = blockIdx.x * kQ + threadIdx.x;
  if (s >= nq) return;
  const uint32_t i = order ? order[s] : s;
  Best b{m2, kNone, kNone};
  const unsigned long long key = (order && nf) ? qkeys[s] : ~0ull;
  if (key != ~0ull) {  // a finite query and a target to search
    double qx, qy, qz;
    load_point(pos, i, qx, qy, qz);
    apply(t, qx, qy, qz);  // the expression of the key kernel: the same bits
    const uint32_t bx = g.bits[0], by = g.bits[1];
    const uint32_t cx = (uint32_t)(key & ((1ull << bx) - 1)), cy = (uint32_t)((key >> bx) & ((1ull << by) - 1)), cz = (uint32_t)(key >> (bx + by));
    // the largest cell distance from the query's cell to a face of the grid: ring rmax is the last one that holds a cell
    uint32_t rmax = cx > g.dim[0] - 1 - cx ? cx : g.dim[0] - 1 - cx;
    rmax = max(rmax, cy > g.dim[1] - 1 - cy ? cy : g.dim[1] - 1 - cy);
    rmax = max(rmax, cz > g.dim[2] - 1 - cz ? cz : g.dim[2] - 1 - cz);
#pragma unroll 1
    for (uint32_t r = 1;; ++r) {
      const uint32_t z0 = cz >= r ? cz - r : 0, z1 = cz + r < g.dim[2] ? cz + r : g.dim[2] - 1;
      const uint32_t y0 = cy >= r ? cy - r : 0, y1 = cy + r < g.dim[1] ? cy + r : g.dim[1] - 1;
      const uint32_t x0 = cx >= r ? cx - r : 0, x1 = cx + r < g.dim[0] ? cx + r : g.dim[0] - 1;
#pragma unroll 1
      for (uint32_t z = z0; z <= z1; ++z) {
        const uint32_t az = z > cz ? z - cz : cz - z;
#pragma unroll 1
        for (uint32_t y = y0; y <= y1; ++y) {
          const uint32_t ay = y > cy ? y - cy : cy - y;
          const unsigned long long row = ((unsigned long long)z << (bx + by)) | ((unsigned long long)y << bx);
          if (r == 1 || az == r || ay == r) {  // a row on the ring's face (ring 1 takes ring 0 along): the whole range
            const uint32_t first = lower_bound(keys, 0, nf, row | x0);
            const uint32_t last = lower_bound(keys, first, nf, (row | x1) + 1);
            scan(xs, ys, zs, tidx, first, last, qx, qy, qz, b);
          } else {  // inside the ring: the two cells at its ends, where the grid has them
            if (cx >= r) {
              const uint32_t first = lower_bound(keys, 0, nf, row | (cx - r));
              const uint32_t last = lower_bound(keys, first, nf, (row | (cx - r)) + 1);
              scan(xs, ys, zs, tidx, first, last, qx, qy, qz, b);
            }
            if (cx + r < g.dim[0]) {
              const uint32_t first = lower_bound(keys, 0, nf, row | (cx + r));
              const uint32_t last = lower_bound(keys, first, nf, (row | (cx + r)) + 1);
              scan(xs, ys, zs, tidx, first, last, qx, qy, qz, b);
            }
          }
        }
      }
      if (r >= rmax) break;
      const double reach = (double)r * g.edge_stop;
      if (b.d2 <= reach * reach) break;
    }
  }
  const bool matched = b.idx != kNone;
  if (out_idx) out_idx[i] = b.idx;
  if (out_dist) out_dist[i] = matched ? __builtin_sqrt(b.d2) : kInf;
  if (out_at) out_at[i] = b.at;
}

__global__ __launch_bounds__(kBlock) void nn_distance_mask_kernel(const double* __restrict__ dist, uint64_t n, double threshold, int keep_far, uint8_t* __restrict__ mask) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const bool near = dist[i] <= threshold;  // false for a NaN and for an unmatched point's +inf against a finite threshold
  mask[i] = (keep_far ? !near : near) ? 1 : 0;
}

// ---- the sums of an ICP step ------------------------------------------------------------------------------------------------------------------
// the device-side record of one step: the first pass leaves the count and the centroids for the second one
using Sums = pstk::NnSums;

// wave: xor tree; block: the waves' sums in wave order.  The result is valid in thread 0.  C counters travel with the N sums (sc: C per wave).
template <int N, int C>
__device__ __forceinline__ void block_sum(double (&v)[N], unsigned long long (&c)[C], double* sv, unsigned long long* sc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] + shfl_xor_any(v[k], off);
#pragma unroll
    for (int k = 0; k < C; ++k) c[k] = c[k] + shfl_xor_any(c[k], off);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sv[wave * N + k] = v[k];
#pragma unroll
    for (int k = 0; k < C; ++k) sc[wave * C + k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = sv[k];
#pragma unroll
    for (int k = 0; k < C; ++k) c[k] = sc[k];
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) {
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = v[k] + sv[w * N + k];
#pragma unroll
      for (int k = 0; k < C; ++k) c[k] = c[k] + sc[w * C + k];
    }
  }
}
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], unsigned long long& c, double* sv, unsigned long long* sc) {
  unsigned long long one[1] = {c};
  block_sum<N, 1>(v, one, sv, sc);
  c = one[0];
}

constexpr int kTerms0 = 6, kTerms1 = 10;  // pass 0: sum (q' - o), sum (p - o); pass 1: H row-major, sum d2

// partials: `blocks` records of N doubles, then `blocks` counts
template <int PASS>
__global__ __launch_bounds__(kBlock) void nn_icp_partial_kernel(Pos pos, uint64_t n, Xform t, const uint32_t* __restrict__ at, const double* __restrict__ xs,
                                                                const double* __restrict__ ys, const double* __restrict__ zs, double ox, double oy, double oz,
                                                                const Sums* __restrict__ rec, double* __restrict__ psum, unsigned long long* __restrict__ pcount) {
  constexpr int N = PASS == 0 ? kTerms0 : kTerms1;
  __shared__ double sv[(kBlock / 64) * N];
  __shared__ unsigned long long sc[kBlock / 64];
  double cq[3] = {0.0, 0.0, 0.0}, cp[3] = {0.0, 0.0, 0.0};
  if constexpr (PASS == 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { cq[a] = rec->cq[a]; cp[a] = rec->cp[a]; }
  }
  const uint64_t first = (uint64_t)blockIdx.x * kRP;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  unsigned long long c = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < kRP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    const uint32_t a = at[i];
    if (a == kNone) continue;
    double qx, qy, qz;
    load_point(pos, i, qx, qy, qz);
    apply(t, qx, qy, qz);
    const double px = xs[a], py = ys[a], pz = zs[a];
    if constexpr (PASS == 0) {
      v[0] = v[0] + (qx - ox); v[1] = v[1] + (qy - oy); v[2] = v[2] + (qz - oz);
      v[3] = v[3] + (px - ox); v[4] = v[4] + (py - oy); v[5] = v[5] + (pz - oz);
    } else {
      const double q[3] = {qx - cq[0], qy - cq[1], qz - cq[2]}, p[3] = {px - cp[0], py - cp[1], pz - cp[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) v[3 * r + s] = v[3 * r + s] + q[r] * p[s];
      const double dx = px - qx, dy = py - qy, dz = pz - qz;
      v[9] = v[9] + ((dx * dx + dy * dy) + dz * dz);
    }
    c += 1;
  }
  block_sum<N>(v, c, sv, sc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) psum[(uint64_t)blockIdx.x * N + k] = v[k];
    pcount[blockIdx.x] = c;
  }
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void nn_icp_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcount, uint64_t blocks, double ox,
                                                              double oy, double oz, Sums* __restrict__ rec) {
  constexpr int N = PASS == 0 ? kTerms0 : kTerms1;
  __shared__ double sv[(kBlock / 64) * N];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t per = (blocks + kRB - 1) / kRB, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  unsigned long long c = 0;
  for (uint64_t b = b0; b < b1; ++b) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] + psum[b * N + k];
    c = c + pcount[b];
  }
  block_sum<N>(v, c, sv, sc);
  if (threadIdx.x != 0) return;
  if constexpr (PASS == 0) {
    const double m = (double)c, o[3] = {ox, oy, oz};
    rec->matched = c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // no match: 0 / 0, and the host answers before it reads them
      rec->cq[a] = o[a] + v[a] / m;
      rec->cp[a] = o[a] + v[3 + a] / m;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) rec->H[k] = v[k];
    rec->sum_d2 = v[9];
  }
}

// ---- the sums of a point-to-plane step --------------------------------------------------------------------------------------------------------
// The normals of the finite targets in the index's sorted order, widened to f64 (exact).  T = double: the [n][3] array of
// pst_compute_normals_device; T = float: a Vec3f32 attribute at any stride and byte offset.
template <typename T>
__global__ __launch_bounds__(kBlock) void nn_gather_normals_kernel(cgptr_t base, uint64_t stride, const uint32_t* __restrict__ order, uint32_t nf, double* __restrict__ nx,
                                                                   double* __restrict__ ny, double* __restrict__ nz) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= nf) return;
  cgptr_t q = base + (uint64_t)order[s] * stride;
  nx[s] = (double)load_un<T>(q); ny[s] = (double)load_un<T>(q + sizeof(T)); nz[s] = (double)load_un<T>(q + 2 * sizeof(T));
}

using PlaneSums = pstk::NnPlaneSums;

// pass 0: sum (q' - o), sum d2 over the used pairs; counters: matched, used.  pass 1: A (21), g (6), sum r^2, sum |w|^2 over the used pairs.
constexpr int kPlaneTerms0 = 4, kPlaneTerms1 = 29, kPlaneCounts = 2;
// position of A[i][k], i <= k, in the row-major upper triangle of a 6 x 6
__host__ __device__ constexpr int tri6(int i, int k) { return i * 6 - i * (i - 1) / 2 + (k - i); }
static_assert(tri6(0, 0) == 0 && tri6(1, 1) == 6 && tri6(5, 5) == 20, "row-major upper triangle");

// a pair is used when its normal is finite and not zero
__device__ __forceinline__ bool usable(double n0, double n1, double n2) {
  return finite(n0) && finite(n1) && finite(n2) && (n0 * n0 + n1 * n1) + n2 * n2 > 0.0;
}

// partials: `blocks` records of N doubles, then `blocks` pairs of counts.  Every accumulator index below is a compile-time constant after
// unrolling: the 29 sums of pass 1 stay in registers.
template <int PASS>
__global__ __launch_bounds__(kBlock) void nn_plane_partial_kernel(Pos pos, uint64_t n, Xform t, const uint32_t* __restrict__ at, const double* __restrict__ xs,
                                                                  const double* __restrict__ ys, const double* __restrict__ zs, const double* __restrict__ nx,
                                                                  const double* __restrict__ ny, const double* __restrict__ nz, double ox, double oy, double oz,
                                                                  const PlaneSums* __restrict__ rec, double* __restrict__ psum, unsigned long long* __restrict__ pcount) {
  constexpr int N = PASS == 0 ? kPlaneTerms0 : kPlaneTerms1;
  __shared__ double sv[(kBlock / 64) * N];
  __shared__ unsigned long long sc[(kBlock / 64) * kPlaneCounts];
  double cq0 = 0.0, cq1 = 0.0, cq2 = 0.0;
  if constexpr (PASS == 1) { cq0 = rec->cq[0]; cq1 = rec->cq[1]; cq2 = rec->cq[2]; }
  const uint64_t first = (uint64_t)blockIdx.x * kRP;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  unsigned long long c[kPlaneCounts] = {0, 0};
#pragma unroll 1
  for (uint32_t j = 0; j < kRP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    const uint32_t a = at[i];
    if (a == kNone) continue;
    c[0] += 1;
    const double n0 = nx[a], n1 = ny[a], n2 = nz[a];
    if (!usable(n0, n1, n2)) continue;
    c[1] += 1;
    double qx, qy, qz;
    load_point(pos, i, qx, qy, qz);
    apply(t, qx, qy, qz);
    const double dx = xs[a] - qx, dy = ys[a] - qy, dz = zs[a] - qz;
    if constexpr (PASS == 0) {
      v[0] = v[0] + (qx - ox); v[1] = v[1] + (qy - oy); v[2] = v[2] + (qz - oz);
      v[3] = v[3] + ((dx * dx + dy * dy) + dz * dz);
    } else {
      const double w0 = qx - cq0, w1 = qy - cq1, w2 = qz - cq2;
      const double jv[6] = {w1 * n2 - w2 * n1, w2 * n0 - w0 * n2, w0 * n1 - w1 * n0, n0, n1, n2};
      const double r = (dx * n0 + dy * n1) + dz * n2;
#pragma unroll
      for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int q = p; q < 6; ++q) v[tri6(p, q)] = v[tri6(p, q)] + jv[p] * jv[q];
        v[21 + p] = v[21 + p] + jv[p] * r;
      }
      v[27] = v[27] + r * r;
      v[28] = v[28] + ((w0 * w0 + w1 * w1) + w2 * w2);
    }
  }
  block_sum<N, kPlaneCounts>(v, c, sv, sc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) psum[(uint64_t)blockIdx.x * N + k] = v[k];
    pcount[2 * (uint64_t)blockIdx.x] = c[0];
    pcount[2 * (uint64_t)blockIdx.x + 1] = c[1];
  }
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void nn_plane_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcount, uint64_t blocks, double ox,
                                                                double oy, double oz, PlaneSums* __restrict__ rec) {
  constexpr int N = PASS == 0 ? kPlaneTerms0 : kPlaneTerms1;
  __shared__ double sv[(kBlock / 64) * N];
  __shared__ unsigned long long sc[(kBlock / 64) * kPlaneCounts];
  const uint64_t per = (blocks + kRB - 1) / kRB, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  unsigned long long c[kPlaneCounts] = {0, 0};
  for (uint64_t b = b0; b < b1; ++b) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] + psum[b * N + k];
    c[0] = c[0] + pcount[2 * b];
    c[1] = c[1] + pcount[2 * b + 1];
  }
  block_sum<N, kPlaneCounts>(v, c, sv, sc);
  if (threadIdx.x != 0) return;
  if constexpr (PASS == 0) {
    const double u = (double)c[1];
    rec->matched = c[0];
    rec->used = c[1];
    rec->cq[0] = ox + v[0] / u;  // no used pair: 0 / 0, and the host answers before it reads them
    rec->cq[1] = oy + v[1] / u;
    rec->cq[2] = oz + v[2] / u;
    rec->sum_d2 = v[3];
  } else {
#pragma unroll
    for (int k = 0; k < 21; ++k) rec->A[k] = v[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) rec->g[k] = v[21 + k];
    rec->sum_r2 = v[27];
    rec->sum_w2 = v[28];
  }
}

}  // namespace

namespace pstk {

bool nn_gather(const Positions& pos, const uint32_t* order, uint32_t nf, double* xs, double* ys, double* zs, hipStream_t stream) {
  if (nf == 0) return true;
  hipLaunchKernelGGL(nn_gather_kernel, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), order, nf, xs, ys, zs);
  return launched();
}

bool nn_count_cells(const unsigned long long* sorted_keys, uint32_t nf, unsigned long long* count, hipStream_t stream) {
  if (hipMemsetAsync(count, 0, sizeof(unsigned long long), stream) != hipSuccess) return false;
  if (nf == 0) return true;
  hipLaunchKernelGGL(nn_count_cells_kernel, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, sorted_keys, nf, count);
  return launched();
}

bool nn_query_keys(const Positions& pos, const NnTransform& t, const NnGrid& g, unsigned long long* keys, uint32_t* vals, hipStream_t stream) {
  hipLaunchKernelGGL(nn_query_key_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, t, g, keys, vals);
  return launched();
}

bool nn_search(const Positions& pos, const NnTransform& t, const NnGrid& g, double m2, const unsigned long long* query_keys, const uint32_t* query_order,
               const unsigned long long* keys, const double* xs, const double* ys, const double* zs, const uint32_t* target_index, uint32_t nf, uint32_t* out_idx,
               double* out_dist, uint32_t* out_at, hipStream_t stream) {
  hipLaunchKernelGGL(nn_search_kernel, dim3(blocks_of(pos.n, kQ)), dim3(kBlock), 0, stream, pos_of(pos), (uint32_t)pos.n, t, g, m2, query_keys, query_order, keys, xs, ys,
                     zs, target_index, nf, out_idx, out_dist, out_at);
  return launched();
}

bool nn_distance_mask(const double* dist, uint64_t n, double threshold, int keep_far, uint8_t* mask, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(nn_distance_mask_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, dist, n, threshold, keep_far, mask);
  return launched();
}

size_t nn_icp_partials_bytes(uint64_t n) { return (size_t)blocks_of(n, kRP) * (kTerms1 + 1) * 8; }

bool nn_icp_sums(const Positions& pos, const NnTransform& t, const uint32_t* at, const double* xs, const double* ys, const double* zs, const double origin[3],
                 void* partials, NnSums* rec, hipStream_t stream) {
  const unsigned blocks = blocks_of(pos.n, kRP);
  double* psum = (double*)partials;
  unsigned long long* pcount = (unsigned long long*)(psum + (size_t)blocks * kTerms1);
  const double ox = origin[0], oy = origin[1], oz = origin[2];
  hipLaunchKernelGGL(nn_icp_partial_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, pos_of(pos), pos.n, t, at, xs, ys, zs, ox, oy, oz, (const NnSums*)rec, psum, pcount);
  hipLaunchKernelGGL(nn_icp_final_kernel<0>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, ox, oy, oz, rec);
  hipLaunchKernelGGL(nn_icp_partial_kernel<1>, dim3(blocks), dim3(kBlock), 0, stream, pos_of(pos), pos.n, t, at, xs, ys, zs, ox, oy, oz, (const NnSums*)rec, psum, pcount);
  hipLaunchKernelGGL(nn_icp_final_kernel<1>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, ox, oy, oz, rec);
  return launched();
}

bool nn_gather_normals(const uint8_t* base, uint64_t stride, bool is_f32, const uint32_t* order, uint32_t nf, double* nx, double* ny, double* nz, hipStream_t stream) {
  if (nf == 0) return true;
  if (is_f32)
    hipLaunchKernelGGL(nn_gather_normals_kernel<float>, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, (cgptr_t)base, stride, order, nf, nx, ny, nz);
  else
    hipLaunchKernelGGL(nn_gather_normals_kernel<double>, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, (cgptr_t)base, stride, order, nf, nx, ny, nz);
  return launched();
}

size_t nn_plane_partials_bytes(uint64_t n) { return (size_t)blocks_of(n, kRP) * (kPlaneTerms1 + kPlaneCounts) * 8; }

bool nn_plane_sums(const Positions& pos, const NnTransform& t, const uint32_t* at, const double* xs, const double* ys, const double* zs, const double* nx,
                   const double* ny, const double* nz, const double origin[3], void* partials, NnPlaneSums* rec, hipStream_t stream) {
  const unsigned blocks = blocks_of(pos.n, kRP);
  double* psum = (double*)partials;
  unsigned long long* pcount = (unsigned long long*)(psum + (size_t)blocks * kPlaneTerms1);
  const double ox = origin[0], oy = origin[1], oz = origin[2];
  hipLaunchKernelGGL(nn_plane_partial_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, pos_of(pos), pos.n, t, at, xs, ys, zs, nx, ny, nz, ox, oy, oz,
                     (const NnPlaneSums*)rec, psum, pcount);
  hipLaunchKernelGGL(nn_plane_final_kernel<0>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, ox, oy, oz, rec);
  hipLaunchKernelGGL(nn_plane_partial_kernel<1>, dim3(blocks), dim3(kBlock), 0, stream, pos_of(pos), pos.n, t, at, xs, ys, zs, nx, ny, nz, ox, oy, oz,
                     (const NnPlaneSums*)rec, psum, pcount);
  hipLaunchKernelGGL(nn_plane_final_kernel<1>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, ox, oy, oz, rec);
  return launched();
}

}  // namespace pstk
