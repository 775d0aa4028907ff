// Region growing: smooth surface patches as connected components over neighbour lists uint32 [n][k] in device memory (the lists of the kNN
// search, or a caller's), normals f64 [n][3] and an optional curvature f64 [n] (include/pasture_amd.h, "Region growing"; tests/region_ref.py
// restates it in numpy).  Every operation is a separately rounded f64 operation (-ffp-contract=off).
//
// Pipeline (region_api.cpp drives it; the host reads one count before the numbering sort).  A point's id is its buffer index throughout:
//   classify  one lane per point: state[i] = 0 (a normal component is not finite), 1 (rim: valid, curvature above the threshold or NaN) or
//             2 (smooth); parent[i] = i; the smooth points are counted with one integer atomic per wave, from the ballot.
//   link      the lists mapped flat, as features.hip maps them: a workgroup owns P = region_points_per_block(k) consecutive points, that is
//             P * k consecutive list elements, and walks them kRegionThreads at a time, so the index reads are coalesced.  The owned points'
//             normals and states are staged in LDS first.  Per slot, cheapest test first: the owner is smooth (LDS), the index is in range and
//             not the owner, the one-byte state[j] == 2; only then the 24-byte gather of the neighbour's normal and the agreement test, then
//             -- when max_distance is finite, which is wave-uniform -- the two positions.  What passes is united.  The lists are not symmetric
//             and need not be: an edge is found from whichever side names the other.  The union-find is that of clusters.hip.
//   attach    launched behind link, so roots are final and nothing is united any more.  A smooth lane looks up its own root.  A rim lane walks
//             its k slots in slot order and takes the root of the first smooth neighbour that counts and agrees, or "none".  Every labelled
//             lane adds to size[root] and folds its index into min_index[root]: the wave-folded tally of grid_index_device.hpp (a ground
//             plane that holds most of the cloud is one address).
//   number    the clusters' numbering in buffer order (cluster_numbering.hpp; the flag, list and rank kernels are those of clusters.hip), then
//             labels and the smooth mask by the one kernel of the numbering that is the regions' own.
//
// No lane ever waits for another lane's write, there is no floating-point atomic, and the only retry loop is the union-find's CAS, which
// strictly descends: sizes are integer sums, the rim choice is "first in slot order", the numbering is a stable sort.
#include "grid_index_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kThreads = pstk::kRegionThreads;
constexpr uint32_t kNone = kNoRoot;
constexpr uint8_t kInvalid = 0, kRim = 1, kSmooth = 2;
static_assert(kThreads == kBlock, "the link kernel is written for one kBlock workgroup");

__device__ __forceinline__ bool agree(double ax, double ay, double az, const double* __restrict__ b, double min_abs_cos) {
  return __builtin_fabs((ax * b[0] + ay * b[1]) + az * b[2]) >= min_abs_cos;
}
// the slot distance of the kNN search, neighbour minus owner; a NaN compares false
__device__ __forceinline__ bool within(const Pos& pos, uint64_t i, uint64_t j, double max_distance) {
  double qx, qy, qz, px, py, pz;
  load_point(pos, i, qx, qy, qz);
  load_point(pos, j, px, py, pz);
  return __builtin_sqrt(squared_distance(px, py, pz, qx, qy, qz)) <= max_distance;
}

// ---- classify ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void region_classify_kernel(const double* __restrict__ normals, const double* __restrict__ curvature, double curvature_threshold,
                                                                 uint32_t n, uint8_t* __restrict__ state, uint32_t* __restrict__ parent,
                                                                 unsigned long long* __restrict__ n_smooth) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool smooth = false;
  if (i < n) {
    const double* v = normals + (uint64_t)i * 3;
    const bool valid = finite(v[0]) && finite(v[1]) && finite(v[2]);
    smooth = valid && (!curvature || curvature[i] <= curvature_threshold);  // (a NaN curvature compares false)
    state[i] = smooth ? kSmooth : valid ? kRim : kInvalid;
    parent[i] = i;
  }
  const uint32_t in_wave = (uint32_t)__builtin_popcountll(__ballot(smooth));
  if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(n_smooth, (unsigned long long)in_wave);
}

// ---- link -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void region_link_kernel(Pos pos, uint32_t n, uint32_t k, uint32_t P, const uint32_t* __restrict__ knn,
                                                               const double* __restrict__ normals, const uint8_t* __restrict__ state, double min_abs_cos,
                                                               double max_distance, uint32_t* parent) {
  extern __shared__ double own_normals[];  // P rows of 3 doubles, then P state bytes
  uint8_t* own_state = (uint8_t*)(own_normals + 3u * P);
  const uint64_t q0 = (uint64_t)blockIdx.x * P;
  const uint32_t points = (uint32_t)(n - q0 < P ? n - q0 : P);
  for (uint32_t l = threadIdx.x; l < 3u * points; l += kThreads) own_normals[l] = normals[q0 * 3 + l];
  for (uint32_t l = threadIdx.x; l < points; l += kThreads) own_state[l] = state[q0 + l];
  __syncthreads();
  const bool limited = max_distance < kInf;  // (uniform: positions are read only then)
  const uint32_t elements = points * k;
  const uint64_t e0 = q0 * k;
  for (uint32_t l = threadIdx.x; l < elements; l += kThreads) {
    const uint32_t p = l / k;
    if (own_state[p] != kSmooth) continue;
    const uint32_t j = knn[e0 + l];
    const uint32_t q = (uint32_t)q0 + p;
    if (j >= n || j == q || state[j] != kSmooth) continue;
    const double* a = own_normals + 3u * p;
    if (!agree(a[0], a[1], a[2], normals + (uint64_t)j * 3, min_abs_cos)) continue;
    if (limited && !within(pos, q, j, max_distance)) continue;
    unite(parent, q, j);
  }
}

// ---- attach + flatten ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void region_attach_kernel(Pos pos, uint32_t n, uint32_t k, const uint32_t* __restrict__ knn, const double* __restrict__ normals,
                                                               const uint8_t* __restrict__ state, double min_abs_cos, double max_distance, uint32_t* parent,
                                                               uint32_t* __restrict__ root, uint32_t* size, uint32_t* min_index) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;  // (no lane leaves before the wave-wide fold at the end)
  uint32_t member = kNone;  // the smooth point whose region i joins
  if (live) {
    const uint8_t st = state[i];
    if (st == kSmooth) {
      member = i;
    } else if (st == kRim) {
      const double* v = normals + (uint64_t)i * 3;
      const double ax = v[0], ay = v[1], az = v[2];
      const bool limited = max_distance < kInf;
      const uint32_t* list = knn + (uint64_t)i * k;
#pragma unroll 1
      for (uint32_t t = 0; t < k; ++t) {
        const uint32_t j = list[t];
        if (j >= n || j == i || state[j] != kSmooth) continue;
        if (limited && !within(pos, i, j, max_distance)) continue;
        if (!agree(ax, ay, az, normals + (uint64_t)j * 3, min_abs_cos)) continue;
        member = j;
        break;
      }
    }
  }
  const uint32_t r = member == kNone ? kNone : find_root(parent, member);  // no union runs any more: what a lane finds IS the root
  if (live) root[i] = r;
  tally_root(r, r != kNone ? i : kNone, size, min_index);
}

// ---- labels (the flag, list and rank kernels of the numbering are the clusters': clusters.hip) ------------------------------------------------------
// rank_of_root: 0xFFFFFFFF where the root's region was dropped; smooth_out is nullable
__global__ __launch_bounds__(kBlock) void region_label_kernel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank_of_root, const uint8_t* __restrict__ state,
                                                              uint32_t n, uint32_t* __restrict__ labels, uint8_t* __restrict__ smooth_out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = root[i];
  labels[i] = r != kNone ? rank_of_root[r] : kNone;
  if (smooth_out) smooth_out[i] = state[i] == kSmooth ? 1 : 0;
}

}  // namespace

namespace pstk {

uint32_t region_points_per_block(uint32_t k) { return k <= 8 ? 256u : k <= 16 ? 128u : k <= 32 ? 64u : 32u; }

bool region_classify(const double* normals, const double* curvature, double curvature_threshold, uint32_t n, uint8_t* state, uint32_t* parent, unsigned long long* n_smooth,
                     hipStream_t stream) {
  hipLaunchKernelGGL(region_classify_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, normals, curvature, curvature_threshold, n, state, parent, n_smooth);
  return launched();
}

bool region_link(const Positions& pos, uint32_t k, const uint32_t* knn, const double* normals, const uint8_t* state, double min_abs_cos, double max_distance,
                 uint32_t* parent, hipStream_t stream) {
  const uint32_t n = (uint32_t)pos.n, P = region_points_per_block(k);
  const size_t lds = (size_t)P * (3 * sizeof(double) + 1);  // 6400 bytes at the most
  hipLaunchKernelGGL(region_link_kernel, dim3(blocks_of(n, P)), dim3(kThreads), lds, stream, pos_of(pos), n, k, P, knn, normals, state, min_abs_cos, max_distance, parent);
  return launched();
}

bool region_attach(const Positions& pos, uint32_t k, const uint32_t* knn, const double* normals, const uint8_t* state, double min_abs_cos, double max_distance,
                   uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream) {
  const uint32_t n = (uint32_t)pos.n;
  if (hipMemsetAsync(size, 0, (size_t)n * sizeof(uint32_t), stream) != hipSuccess || hipMemsetAsync(min_index, 0xFF, (size_t)n * sizeof(uint32_t), stream) != hipSuccess)
    return false;
  hipLaunchKernelGGL(region_attach_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), n, k, knn, normals, state, min_abs_cos, max_distance, parent,
                     root, size, min_index);
  return launched();
}

bool region_labels(const uint32_t* root, const uint32_t* rank_of_root, const uint8_t* state, uint32_t n, uint32_t* labels, uint8_t* smooth_out, hipStream_t stream) {
  hipLaunchKernelGGL(region_label_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, root, rank_of_root, state, n, labels, smooth_out);
  return launched();
}

}  // namespace pstk
