// Euclidean cluster extraction: connected components of the graph "two finite points are adjacent iff (dx*dx + dy*dy) + dz*dz <= t2"
// (include/pasture_amd.h, "Euclidean cluster extraction"; every operation a separately rounded f64 operation, no sqrt).
//
// Pipeline (clusters_api.cpp drives it; the host reads two small records in between):
//   bounds    AABB over the FINITE points and their number: block folds, then integer atomicMin / atomicMax on an order-preserving encoding
//   keys      cell key per point on a uniform grid, x in the lowest bits: key = (cz << (bx + by)) | (cy << bx) | cx; non-finite points get the
//             all-ones key.  The 64-bit radix sort orders (key, index) on bits [0, bx + by + bz + 1): bit bx + by + bz is 0 in every finite key
//             and 1 in the all-ones key, so the non-finite points end up behind the nf finite ones.
//   gather    positions into sorted order (three f64 arrays), parent[s] = s.  From here on a point's id is its SORTED position s < nf.
//   traverse  the hot kernel, one lane per point: every candidate of LOWER id in the 3 x 3 x 3 stencil is tested and, when adjacent, united.
//             Lower ids have lower or equal keys, so only five of the nine (y, z) rows can hold any: the four rows that sort before the point's
//             own -- each one contiguous key range [x - 1, x + 1], found by two binary searches of the sorted keys -- and the own row up to the
//             point itself.  Lanes of a wave are neighbours in the sorted order: they search the same ranges and read the same candidates.
//   flatten   root per point, points per root and smallest buffer index per root: the wave-folded tally of grid_index_device.hpp
//   number    size filter, flag the smallest member of every kept component, exclusive scan (= the kept roots in ascending smallest-member
//             order), one stable sort on 0xFFFFFFFF - size (ties keep that order), ranks back to the roots, labels to the points.  The flag,
//             list and rank kernels below serve DBSCAN and the regions as well; cluster_numbering.hpp holds the host sequence for all three.
//
// The grid's cell edge is STRICTLY larger than the tolerance, by the relative margin 2^-20 (cluster_grid.hpp makes it, and doubles it until no
// axis has more than 2^21 - 1 cells).  Why that is enough for "adjacent points are at most one cell apart on every axis": adjacency gives
// dx*dx <= t2 up to the roundings of the sum, so |xj - xi| <= tolerance * (1 + 2^-50).  The cell number is trunc(q), q = fl(fl(x - min) / edge):
// two roundings, so q is within the relative error 2^-52 of the exact (x - min) / edge, which is below 2^21: an absolute error below 2^-31 each.
// Exact quotients of adjacent points differ by at most tolerance * (1 + 2^-50) / (tolerance * (1 + 2^-20)) < 1 - 2^-21; the computed ones by less
// than 1 - 2^-21 + 2^-30 < 1, and two numbers less than 1 apart truncate to cell numbers at most 1 apart.  With an edge EQUAL to the tolerance
// the bound would be 1 + 2^-30: two points exactly `tolerance` apart can land two cells apart and the stencil would miss the pair.
//
// Union-find, lock-free: find both roots, atomicCAS the larger root's parent from itself to the smaller root, on failure go on from what the CAS
// returned.  parent[v] <= v always and only ever decreases (the path halving is an atomicMin), so every retry starts strictly lower: no locks,
// no lane ever waits for another lane's write.  The parent reads inside the kernel are agent-scope relaxed loads; a read that is stale (the
// XCDs' L2s are not coherent) still returns a former parent, which is a member of the same set with a lower id, so it costs steps, never
// correctness: only the CAS decides who is a root, and it executes at the memory side.
#include "grid_index_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kClusterPointsPerBlock;
constexpr uint32_t kBoundsPoints = 1024;  // points per workgroup of the bounds fold, four per lane
constexpr uint32_t kNone = kNoRoot;
static_assert(kP == kBlock, "one lane per point");

using Record = pstk::ClusterRecord;
using Grid = pstk::ClusterGrid;

__device__ __forceinline__ uint32_t cell_of(double v, double mn, double edge, uint32_t dim) {
  const double q = (v - mn) / edge;
  const uint32_t c = (uint32_t)q;             // 0 <= q < 2^21: the conversion truncates
  return c < dim ? c : dim - 1;               // (never taken: the host sized dim from the largest coordinate with the same expression)
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cluster_bounds_kernel(Pos pos, uint64_t n, Record* __restrict__ rec) {
  __shared__ double scratch[4 * 2 * 3];
  const uint64_t first = (uint64_t)blockIdx.x * kBoundsPoints;
  double mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
  unsigned long long count = 0;
#pragma unroll
  for (uint32_t j = 0; j < kBoundsPoints / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i < n) {
      double x, y, z;
      load_point(pos, i, x, y, z);
      if (finite(x) && finite(y) && finite(z)) {
        mn[0] = fold_min(mn[0], x); mn[1] = fold_min(mn[1], y); mn[2] = fold_min(mn[2], z);
        mx[0] = fold_max(mx[0], x); mx[1] = fold_max(mx[1], y); mx[2] = fold_max(mx[2], z);
        count += 1;
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) count += shfl_xor_any(count, off);
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(&rec->finite_count, count);
  block_reduce_minmax<double, 3>(mn, mx, scratch);
  if (threadIdx.x == 0 && mn[0] <= mx[0]) {  // the block holds a finite point
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&rec->min_ordered[a], ordered(mn[a]));
      atomicMax(&rec->max_ordered[a], ordered(mx[a]));
    }
  }
}

// ---- keys, gather -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cluster_key_kernel(Pos pos, uint64_t n, Grid g, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  load_point(pos, i, x, y, z);
  unsigned long long key = ~0ull;
  if (finite(x) && finite(y) && finite(z)) {
    const unsigned long long cx = cell_of(x, g.min[0], g.edge, g.dim[0]), cy = cell_of(y, g.min[1], g.edge, g.dim[1]), cz = cell_of(z, g.min[2], g.edge, g.dim[2]);
    key = (cz << (g.bits[0] + g.bits[1])) | (cy << g.bits[0]) | cx;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void cluster_gather_kernel(Pos pos, const uint32_t* __restrict__ order, uint32_t nf, double* __restrict__ xs, double* __restrict__ ys,
                                                                double* __restrict__ zs, uint32_t* __restrict__ parent) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= nf) return;
  double x, y, z;
  load_point(pos, order[s], x, y, z);
  xs[s] = x; ys[s] = y; zs[s] = z;
  parent[s] = s;
}

// ---- the traversal (the union-find, the binary search, the stencil rows and the predicate: grid_index_device.hpp) -------------------------------
__global__ __launch_bounds__(kBlock) void cluster_traverse_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ xs, const double* __restrict__ ys,
                                                                  const double* __restrict__ zs, uint32_t nf, Grid g, double t2, uint32_t* parent) {
  const uint32_t s = blockIdx.x * kP + threadIdx.x;
  if (s >= nf) return;
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
      if (squared_distance(xs[c], ys[c], zs[c], px, py, pz) <= t2) unite(parent, s, c);
  }
}

// ---- flatten and numbering ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cluster_flatten_kernel(uint32_t* parent, const uint32_t* __restrict__ order, uint32_t nf, uint32_t* __restrict__ root,
                                                                 uint32_t* size, uint32_t* min_index) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  const bool live = s < nf;  // (no lane leaves before the wave-wide tally)
  const uint32_t r = live ? find_root(parent, s) : kNone;  // no union runs any more: what a lane finds IS the root
  if (live) root[s] = r;
  tally_root(r, live ? order[s] : kNone, size, min_index);
}

// The smallest member of every kept component is flagged and remembers its root.  Ids are sorted positions (clusters, DBSCAN) or buffer
// indices (regions); only a root has root[id] == id.  DBSCAN keeps everything: min_size 1, max_size all ones.
__global__ __launch_bounds__(kBlock) void cluster_flag_kernel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ size, const uint32_t* __restrict__ min_index,
                                                              uint32_t n_ids, unsigned long long min_size, unsigned long long max_size, uint32_t* __restrict__ flags,
                                                              uint32_t* __restrict__ root_at, unsigned long long* __restrict__ n_labelled) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_ids || root[s] != s) return;
  const unsigned long long sz = size[s];
  if (sz < min_size || sz > max_size) return;
  flags[min_index[s]] = 1;
  root_at[min_index[s]] = s;
  atomicAdd(n_labelled, sz);
}

__global__ __launch_bounds__(kBlock) void cluster_list_kernel(const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ offsets,
                                                              const uint32_t* __restrict__ root_at, const uint32_t* __restrict__ size, uint64_t n,
                                                              uint32_t* __restrict__ list_keys, uint32_t* __restrict__ list_roots) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const unsigned long long p = offsets[i];
  const uint32_t r = root_at[i];
  list_keys[p] = kNone - size[r];
  list_roots[p] = r;
}

__global__ __launch_bounds__(kBlock) void cluster_rank_kernel(const uint32_t* __restrict__ sorted_keys, const uint32_t* __restrict__ sorted_roots, uint32_t kept,
                                                              uint32_t* __restrict__ rank_of_root, unsigned long long* __restrict__ sizes) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= kept) return;
  rank_of_root[sorted_roots[c]] = c;
  sizes[c] = kNone - sorted_keys[c];
}

__global__ __launch_bounds__(kBlock) void cluster_label_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank_of_root,
                                                               uint64_t n, uint32_t nf, uint32_t* __restrict__ labels) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  labels[order[s]] = s < nf ? rank_of_root[root[s]] : kNone;  // (the non-finite points sorted behind the finite ones; a dropped root: all ones)
}

__global__ __launch_bounds__(kBlock) void cluster_mask_kernel(const uint32_t* __restrict__ labels, uint64_t n, uint32_t first, uint32_t count, uint8_t* __restrict__ mask) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = labels[i];
  mask[i] = (l != kNone && l >= first && l - first < count) ? 1 : 0;  // l - first cannot wrap behind l >= first
}

}  // namespace

namespace pstk {

bool cluster_bounds(const Positions& pos, ClusterRecord* rec, hipStream_t stream) {
  // min: all ones, max / counts: zero -- the identities of the ordered encoding
  if (hipMemsetAsync(rec, 0, sizeof(ClusterRecord), stream) != hipSuccess || hipMemsetAsync(rec->min_ordered, 0xFF, sizeof(rec->min_ordered), stream) != hipSuccess)
    return false;
  hipLaunchKernelGGL(cluster_bounds_kernel, dim3(blocks_of(pos.n, kBoundsPoints)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, rec);
  return launched();
}

double cluster_decode_ordered(unsigned long long v) { return decode_ordered(v); }

bool cluster_keys(const Positions& pos, const ClusterGrid& g, unsigned long long* keys, uint32_t* vals, hipStream_t stream) {
  hipLaunchKernelGGL(cluster_key_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, g, keys, vals);
  return launched();
}

bool cluster_components(const Positions& pos, const ClusterGrid& g, double t2, const unsigned long long* sorted_keys, const uint32_t* order, uint32_t nf, double* xs,
                        double* ys, double* zs, uint32_t* parent, hipStream_t stream, hipEvent_t gathered) {
  hipLaunchKernelGGL(cluster_gather_kernel, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), order, nf, xs, ys, zs, parent);
  if (gathered && hipEventRecord(gathered, stream) != hipSuccess) return false;
  hipLaunchKernelGGL(cluster_traverse_kernel, dim3(blocks_of(nf, kP)), dim3(kBlock), 0, stream, sorted_keys, (const double*)xs, (const double*)ys, (const double*)zs, nf, g,
                     t2, parent);
  return launched();
}

bool cluster_flatten(uint32_t* parent, const uint32_t* order, uint32_t nf, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream) {
  if (hipMemsetAsync(size, 0, (size_t)nf * sizeof(uint32_t), stream) != hipSuccess || hipMemsetAsync(min_index, 0xFF, (size_t)nf * sizeof(uint32_t), stream) != hipSuccess)
    return false;
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks_of(nf, kBlock)), dim3(kBlock), 0, stream, parent, order, nf, root, size, min_index);
  return launched();
}

bool cluster_flag_kept(const uint32_t* root, const uint32_t* size, const uint32_t* min_index, uint64_t n, uint32_t n_ids, uint64_t min_size, uint64_t max_size,
                       uint32_t* flags, uint32_t* root_at, unsigned long long* n_labelled, hipStream_t stream) {
  if (hipMemsetAsync(flags, 0, (size_t)(n + 1) * sizeof(uint32_t), stream) != hipSuccess) return false;  // (one flag more: the scan's last offset is the total)
  hipLaunchKernelGGL(cluster_flag_kernel, dim3(blocks_of(n_ids, kBlock)), dim3(kBlock), 0, stream, root, size, min_index, n_ids, (unsigned long long)min_size,
                     (unsigned long long)max_size, flags, root_at, n_labelled);
  return launched();
}

bool cluster_list_kept(const uint32_t* flags, const unsigned long long* offsets, const uint32_t* root_at, const uint32_t* size, uint64_t n, uint32_t* list_keys,
                       uint32_t* list_roots, hipStream_t stream) {
  hipLaunchKernelGGL(cluster_list_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, flags, offsets, root_at, size, n, list_keys, list_roots);
  return launched();
}

bool cluster_ranks(const uint32_t* sorted_keys, const uint32_t* sorted_roots, uint32_t kept, uint32_t n_ids, uint32_t* rank_of_root, unsigned long long* sizes,
                   hipStream_t stream) {
  if (hipMemsetAsync(rank_of_root, 0xFF, (size_t)n_ids * sizeof(uint32_t), stream) != hipSuccess) return false;
  if (kept) hipLaunchKernelGGL(cluster_rank_kernel, dim3(blocks_of(kept, kBlock)), dim3(kBlock), 0, stream, sorted_keys, sorted_roots, kept, rank_of_root, sizes);
  return launched();
}

bool cluster_labels(const uint32_t* order, const uint32_t* root, const uint32_t* rank_of_root, uint64_t n, uint32_t nf, uint32_t* labels, hipStream_t stream) {
  hipLaunchKernelGGL(cluster_label_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, order, root, rank_of_root, n, nf, labels);
  return launched();
}

bool cluster_mask(const uint32_t* labels, uint64_t n, uint32_t first_cluster, uint32_t cluster_count, uint8_t* mask, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(cluster_mask_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, labels, n, first_cluster, cluster_count, mask);
  return launched();
}

}  // namespace pstk
