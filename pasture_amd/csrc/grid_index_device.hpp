// What the consumers of the cluster index and of the union-find share in their kernels (clusters.hip, sample.hip, dbscan.hip, region.hip): the
// lock-free union-find over ids (the argument for it is at the head of clusters.hip), the wave-folded tally of sizes and smallest members per
// root, the binary search of the sorted cell keys, the rows of the 3 x 3 x 3 stencil and the pair predicate.
#pragma once
#include "positions_device.hpp"

namespace pstd {

// ---- union-find -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of v's set as far as this lane can see, halving the path on the way: every value stored is an ancestor, and below what it replaces
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t v) {
  for (;;) {
    const uint32_t p = parent_of(parent, v);
    if (p == v) return v;
    const uint32_t gp = parent_of(parent, p);
    if (gp == p) return p;
    atomicMin(parent + v, gp);
    v = gp;
  }
}
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return;
    a = seen;  // hi is no root any more: its parent `seen` < hi is where the search goes on -- strictly lower every time round
    b = lo;
  }
}

// ---- the tally: members per root and the smallest member of every root ---------------------------------------------------------------------------
constexpr uint32_t kNoRoot = 0xFFFFFFFFu;
constexpr uint32_t kFoldRounds = 4;  // distinct roots per wave whose members are folded in the wave before anything is sent
// size[r] += 1 and min_index[r] = min(min_index[r], mine) for the lane's final root r (no union runs any more), `mine` the index the caller
// numbers by.  EVERY lane of the wave must get here: a lane with nothing to add -- past the end, noise, invalid -- passes r == kNoRoot.
// Lanes of a wave are neighbours and mostly share a root, and a component that holds most of the cloud would take one atomic per point on
// ONE address, which the memory side serves one after the other.  So the lanes that share the root of the first pending lane fold their
// count and their smallest index in the wave and send one pair of atomics; after kFoldRounds distinct roots the lanes still pending send
// their own.  Integer sums and minima: the result does not depend on the grouping.
__device__ __forceinline__ void tally_root(uint32_t r, uint32_t mine, uint32_t* size, uint32_t* min_index) {
  bool pending = r != kNoRoot;
#pragma unroll 1
  for (uint32_t round = 0; round < kFoldRounds; ++round) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;  // (wave-uniform)
    const int leader = __builtin_ctzll(todo);
    const uint32_t r0 = (uint32_t)__shfl((int)r, leader, 64);
    const bool same = pending && r == r0;
    const uint32_t members = (uint32_t)__builtin_popcountll(__ballot(same));
    uint32_t lowest = same ? mine : kNoRoot;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t other = shfl_xor_any(lowest, off);
      lowest = other < lowest ? other : lowest;
    }
    if ((int)(threadIdx.x & 63) == leader) {
      atomicAdd(size + r0, members);
      atomicMin(min_index + r0, lowest);
    }
    pending = pending && !same;
  }
  if (pending) {
    atomicAdd(size + r, 1u);
    atomicMin(min_index + r, mine);
  }
}

// ---- the sorted keys and the 3 x 3 x 3 stencil -------------------------------------------------------------------------------------------------

// first position in keys[0, end) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const unsigned long long* __restrict__ keys, uint32_t end, unsigned long long k) {
  uint32_t lo = 0, hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the cell of a sorted key and the clamped x range of its stencil
struct Cell { uint32_t cx, cy, cz, x0, x1; };
__device__ __forceinline__ Cell cell_of_key(unsigned long long key, const pstk::ClusterGrid& g) {
  const uint32_t bx = g.bits[0], by = g.bits[1];
  Cell c;
  c.cx = (uint32_t)(key & ((1ull << bx) - 1));
  c.cy = (uint32_t)((key >> bx) & ((1ull << by) - 1));
  c.cz = (uint32_t)(key >> (bx + by));
  c.x0 = c.cx > 0 ? c.cx - 1 : 0;
  c.x1 = c.cx + 1 < g.dim[0] ? c.cx + 1 : c.cx;
  return c;
}
// the (y, z) row dz, dy cells away: false when it lies outside the grid, else the key of its cell x = 0.  With x in the lowest bits the cells
// x0 .. x1 of a row are ONE contiguous key range, [row | x0, (row | x1) + 1)
__device__ __forceinline__ bool stencil_row(const Cell& c, const pstk::ClusterGrid& g, int dz, int dy, unsigned long long& row) {
  if ((dz < 0 && c.cz == 0) || (dz > 0 && c.cz + 1 >= g.dim[2]) || (dy < 0 && c.cy == 0) || (dy > 0 && c.cy + 1 >= g.dim[1])) return false;
  row = ((unsigned long long)(c.cz + dz) << (g.bits[0] + g.bits[1])) | ((unsigned long long)(c.cy + dy) << g.bits[0]);
  return true;
}

// The row loops themselves stay written out in the kernels, in two shapes: the five rows that can hold candidates of LOWER id than a sorted
// point s -- lower ids have lower or equal keys: in key order (z - 1, y - 1), (z - 1, y), (z - 1, y + 1), (z, y - 1), then the own row, which
// ends at s (cluster_traverse_kernel, dbscan_link_kernel) -- and all nine rows, row r being r / 3 - 1 in z and r % 3 - 1 in y, with or
// without an early stop (dbscan_count_kernel, dbscan_border_kernel, sample_decide_kernel).  Folded into walkers that take a callable, the
// early stop of the decision kernel costs seven SGPRs more, and with them one wave per SIMD.

// the pair predicate's left side, candidate minus point: three subtractions, three products and two sums, each rounded on its own, in this order
__device__ __forceinline__ double squared_distance(double cx, double cy, double cz, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double dx = cx - px, dy = cy - py, dz = cz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace pstd
