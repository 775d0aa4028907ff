// What the consumers of the cluster index share in their kernels (clusters.hip, sample.hip, dbscan.hip): the binary search of the sorted cell
// keys and the lock-free union-find over sorted positions (the argument for it is at the head of clusters.hip).
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

// first position in keys[0, end) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const unsigned long long* __restrict__ keys, uint32_t end, unsigned long long k) {
  uint32_t lo = 0, hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace pstd
