// DBSCAN: core, border and noise points over the neighbour relation "(dx*dx + dy*dy) + dz*dz <= e2" (include/pasture_amd.h, "DBSCAN"; every
// operation a separately rounded f64 operation, no sqrt -- the adjacency of clusters.hip and the conflict of sample.hip).
//
// Pipeline (dbscan_api.cpp drives it; the host reads one small record after the bounds and one count before the numbering sort):
//   index     the clusters' own: cluster_bounds, cluster_keys on a grid whose cell edge is STRICTLY above eps by the relative margin 2^-20, the
//             64-bit radix sort, the positions gathered into sorted order.  The argument at the head of clusters.hip carries over unchanged:
//             neighbours are at most one cell apart on every axis.  From here on a point's id is its SORTED position s < nf.
//   count     one lane per point: all nine (y, z) rows of the 3 x 3 x 3 stencil, each one contiguous key range [x - 1, x + 1] found by two
//             binary searches of the sorted keys (the walk of sample.hip's decision kernel).  The lane counts the candidates that pass the
//             predicate -- itself among them -- and stops when the count reaches min_points: core[s] = 1.  It also sets parent[s] = s.
//   link      the cluster traversal restricted to core points: the five rows that hold candidates of lower id, unite(s, c) only when both are
//             core and neighbours.  A lane that is not core returns at once.  The union-find is that of clusters.hip.
//   border    launched behind the link kernel, so roots are final and nothing is united any more.  A core lane looks up its root.  A lane that
//             is not core walks the nine rows for core neighbours and keeps the smallest (d2, buffer index); it takes that core point's root,
//             or "none" without one.  Every labelled lane adds to size[root] and folds its buffer index into min_index[root]: the wave-folded
//             tally of grid_index_device.hpp (a cluster of most of the cloud is one address).
//   number    the clusters' numbering with a filter that keeps everything (cluster_numbering.hpp; the flag, list and rank kernels are those
//             of clusters.hip), then labels and core flags scattered to buffer order by the one kernel of the numbering that is DBSCAN's own.
//
// The cell of a key, the stencil rows, the binary search, the predicate, the union-find and the tally are grid_index_device.hpp's, shared with
// clusters.hip and sample.hip; the row loops are written out here (why: there).
// Lanes of a wave are neighbours in the sorted order: in all three kernels they search the same key ranges and read the same candidates.  No
// lane ever waits for another lane's write, and there is no floating-point atomic: sizes are integer sums, the border choice is a minimum over
// a set that does not depend on the order it is walked in.
#include "grid_index_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kDbscanPointsPerBlock;
constexpr uint32_t kNone = kNoRoot;
static_assert(kP == kBlock, "one lane per point");

using Grid = pstk::ClusterGrid;

// ---- count ------------------------------------------------------------------------------------------------------------------------------------
// min_points <= nf (the host answers a larger one itself), so it fits 32 bits
__global__ __launch_bounds__(kBlock) void dbscan_count_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ xs, const double* __restrict__ ys,
                                                              const double* __restrict__ zs, uint32_t nf, Grid g, double e2, uint32_t min_points,
                                                              uint8_t* __restrict__ core, uint32_t* __restrict__ parent, unsigned long long* __restrict__ n_core) {
  const uint32_t s = blockIdx.x * kP + threadIdx.x;
  bool is_core = false;
  if (s < nf) {
    const Cell cell = cell_of_key(keys[s], g);
    const double px = xs[s], py = ys[s], pz = zs[s];
    uint32_t count = 0;
#pragma unroll 1
    for (int r = 0; r < 9 && count < min_points; ++r) {
      unsigned long long row;
      if (!stencil_row(cell, g, r / 3 - 1, r % 3 - 1, row)) continue;
      const uint32_t first = lower_bound(keys, nf, row | cell.x0);
      const uint32_t last = lower_bound(keys, nf, (row | cell.x1) + 1);
      for (uint32_t c = first; c < last && count < min_points; ++c)  // (c == s passes: a point is its own neighbour)
        if (squared_distance(xs[c], ys[c], zs[c], px, py, pz) <= e2) ++count;
    }
    is_core = count >= min_points;
    core[s] = is_core ? 1 : 0;
    parent[s] = s;
  }
  const uint32_t in_wave = (uint32_t)__builtin_popcountll(__ballot(is_core));
  if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(n_core, (unsigned long long)in_wave);
}

// ---- link -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dbscan_link_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ xs, const double* __restrict__ ys,
                                                             const double* __restrict__ zs, const uint8_t* __restrict__ core, uint32_t nf, Grid g, double e2,
                                                             uint32_t* parent) {
  const uint32_t s = blockIdx.x * kP + threadIdx.x;
  if (s >= nf || !core[s]) return;
  const Cell cell = cell_of_key(keys[s], g);
  const double px = xs[s], py = ys[s], pz = zs[s];
  // rows in key order below the own one: (z - 1, y - 1), (z - 1, y), (z - 1, y + 1), (z, y - 1); then the own row, which ends at s
#pragma unroll 1
  for (int r = 0; r < 5; ++r) {
    unsigned long long row;
    if (!stencil_row(cell, g, r < 3 ? -1 : 0, r < 3 ? r - 1 : r - 4, row)) continue;
    const uint32_t first = lower_bound(keys, s, row | cell.x0);
    const uint32_t last = r == 4 ? s : lower_bound(keys, s, (row | cell.x1) + 1);  // (keys below s only: every candidate has a lower id)
    for (uint32_t c = first; c < last; ++c)
      if (core[c] && squared_distance(xs[c], ys[c], zs[c], px, py, pz) <= e2) unite(parent, s, c);
  }
}

// ---- border + flatten ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dbscan_border_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ xs, const double* __restrict__ ys,
                                                               const double* __restrict__ zs, const uint8_t* __restrict__ core, const uint32_t* __restrict__ order,
                                                               uint32_t nf, Grid g, double e2, uint32_t* parent, uint32_t* __restrict__ root, uint32_t* size,
                                                               uint32_t* min_index) {
  const uint32_t s = blockIdx.x * kP + threadIdx.x;
  const bool live = s < nf;  // (no lane leaves before the wave-wide tally at the end)
  uint32_t member = live ? s : kNone;  // the core point whose cluster s joins
  if (live && !core[s]) {
    const Cell cell = cell_of_key(keys[s], g);
    const double px = xs[s], py = ys[s], pz = zs[s];
    double best_d2 = kInf;  // (every neighbour's d2 is finite: it is <= e2)
    uint32_t best_index = kNone;
    member = kNone;
#pragma unroll 1
    for (int r = 0; r < 9; ++r) {
      unsigned long long row;
      if (!stencil_row(cell, g, r / 3 - 1, r % 3 - 1, row)) continue;
      const uint32_t first = lower_bound(keys, nf, row | cell.x0);
      const uint32_t last = lower_bound(keys, nf, (row | cell.x1) + 1);
      for (uint32_t c = first; c < last; ++c) {
        if (!core[c]) continue;
        const double d2 = squared_distance(xs[c], ys[c], zs[c], px, py, pz);
        if (!(d2 <= e2) || d2 > best_d2) continue;
        const uint32_t index = order[c];
        if (d2 < best_d2 || index < best_index) {
          best_d2 = d2;
          best_index = index;
          member = c;
        }
      }
    }
  }
  const uint32_t r = member == kNone ? kNone : find_root(parent, member);  // no union runs any more: what a lane finds IS the root
  if (live) root[s] = r;
  tally_root(r, r != kNone ? order[s] : kNone, size, min_index);
}

// ---- labels (the flag, list and rank kernels of the numbering are the clusters': clusters.hip) ------------------------------------------------------
// labels and core flags to buffer order; core_out is nullable
__global__ __launch_bounds__(kBlock) void dbscan_label_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank_of_root,
                                                              const uint8_t* __restrict__ core, uint64_t n, uint32_t nf, uint32_t* __restrict__ labels,
                                                              uint8_t* __restrict__ core_out) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  const uint32_t i = order[s];
  uint32_t label = kNone;  // (the non-finite points sorted behind the finite ones)
  if (s < nf) {
    const uint32_t r = root[s];
    if (r != kNone) label = rank_of_root[r];
  }
  labels[i] = label;
  if (core_out) core_out[i] = s < nf ? core[s] : 0;
}

}  // namespace

namespace pstk {

bool dbscan_count(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, uint32_t nf, const ClusterGrid& g, double e2,
                  uint32_t min_points, uint8_t* core, uint32_t* parent, unsigned long long* n_core, hipStream_t stream) {
  hipLaunchKernelGGL(dbscan_count_kernel, dim3(blocks_of(nf, kP)), dim3(kBlock), 0, stream, sorted_keys, xs, ys, zs, nf, g, e2, min_points, core, parent, n_core);
  return launched();
}

bool dbscan_link(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint8_t* core, uint32_t nf, const ClusterGrid& g,
                 double e2, uint32_t* parent, hipStream_t stream) {
  hipLaunchKernelGGL(dbscan_link_kernel, dim3(blocks_of(nf, kP)), dim3(kBlock), 0, stream, sorted_keys, xs, ys, zs, core, nf, g, e2, parent);
  return launched();
}

bool dbscan_border(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint8_t* core, const uint32_t* order, uint32_t nf,
                   const ClusterGrid& g, double e2, uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream) {
  if (hipMemsetAsync(size, 0, (size_t)nf * sizeof(uint32_t), stream) != hipSuccess || hipMemsetAsync(min_index, 0xFF, (size_t)nf * sizeof(uint32_t), stream) != hipSuccess)
    return false;
  hipLaunchKernelGGL(dbscan_border_kernel, dim3(blocks_of(nf, kP)), dim3(kBlock), 0, stream, sorted_keys, xs, ys, zs, core, order, nf, g, e2, parent, root, size, min_index);
  return launched();
}

bool dbscan_labels(const uint32_t* order, const uint32_t* root, const uint32_t* rank_of_root, const uint8_t* core, uint64_t n, uint32_t nf, uint32_t* labels,
                   uint8_t* core_out, hipStream_t stream) {
  hipLaunchKernelGGL(dbscan_label_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, order, root, rank_of_root, core, n, nf, labels, core_out);
  return launched();
}

}  // namespace pstk
