// The sign of a bound that is +-0 (device side of pstk::ZeroScan).
//
// The reference folds in index order with strict compares (bounds.rs:30-85, math/minmax.rs:78-94, raw_writers.rs:28-48), so among equal values the
// FIRST one stays: min([+0, -0]) = +0, min([-0, +0]) = -0.  v_min_f64 / v_max_f64 do not see index order, so the folds here stay as they are and,
// when a bound comes out as +-0, the last fold kernel looks up the first zero of that component and takes its bits.  No zero bound: one LDS word
// and a barrier.
#pragma once
#include "device_common.hpp"
#include "kernels.hpp"

namespace pstd {

// Every thread of the block: hit[c] = the first index e < s.n whose component c is +-0, for the components in `need` (bit c); ~0 where there is
// none.  Chunks of U * BLK elements in index order; stops after the chunk that holds the last component's first zero.
template <typename S, int NV, int BLK = kBlock>
__device__ __forceinline__ void first_zero_scan(const pstk::ZeroScan& s, uint32_t need, unsigned long long* hit) {
  constexpr int U = 32;
  cgptr_t base = (cgptr_t)s.base;
  for (uint64_t chunk = 0; need != 0 && chunk < s.n; chunk += (uint64_t)U * BLK) {
    int any = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (!((need >> c) & 1u)) continue;
      S v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t e = chunk + (uint64_t)u * BLK + threadIdx.x;
        v[u] = e < s.n ? load_un<S>(base + e * s.stride + c * sizeof(S)) : (S)1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (v[u] == (S)0) {
          atomicMin(&hit[c], (unsigned long long)(chunk + (uint64_t)u * BLK + threadIdx.x));
          any = 1;
        }
    }
    if (__syncthreads_or(any)) {
#pragma unroll
      for (int c = 0; c < NV; ++c)
        if (hit[c] != ~0ull) need &= ~(1u << c);
      __syncthreads();  // every thread has read hit[] before the next chunk can lower it
    }
  }
}

// Every thread of the block; mn / mx hold the folded bounds in thread 0 (block_reduce_minmax).  A bound that is +-0 takes the bits of the first
// zero of its component in the scanned elements (components of type S at s.base + e * s.stride).  settled (thread 0): bit c = min c, bit NV + c =
// max c is already final (a seed that comes before every element, see las_encode_fold_kernel).
template <typename S, typename T, int NV, int BLK = kBlock>
__device__ __forceinline__ void zero_bounds_in_index_order(const pstk::ZeroScan& s, T (&mn)[NV], T (&mx)[NV], uint32_t settled = 0) {
  __shared__ uint32_t want_s;
  __shared__ unsigned long long hit[NV];
  if (threadIdx.x == 0) {
    uint32_t want = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      hit[c] = ~0ull;
      if (mn[c] == (T)0) want |= 1u << c;
      if (mx[c] == (T)0) want |= 1u << (NV + c);
    }
    want_s = s.n ? (want & ~settled) : 0u;
  }
  __syncthreads();
  const uint32_t want = want_s;
  if (want == 0) return;
  first_zero_scan<S, NV, BLK>(s, (want | (want >> NV)) & ((1u << NV) - 1u), hit);
  __syncthreads();
  if (threadIdx.x == 0) {
    cgptr_t base = (cgptr_t)s.base;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (hit[c] == ~0ull) continue;
      const T z = (T)load_un<S>(base + hit[c] * s.stride + c * sizeof(S));
      if ((want >> c) & 1u) mn[c] = z;
      if ((want >> (NV + c)) & 1u) mx[c] = z;
    }
  }
}

}  // namespace pstd
