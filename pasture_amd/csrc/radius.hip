// Fixed-radius neighbour search over a pst_nn_index: per-query counts and CSR lists (include/pasture_amd.h, "Fixed-radius neighbour search").
//
// Definitions.  A query q is first sent through the optional transform exactly as in nn.hip, x' = ((r00*x + r01*y) + r02*z) + t0.  A finite target
// p is a NEIGHBOUR iff d2 = (dx*dx + dy*dy) + dz*dz <= r2, dx = p.x - q'.x, r2 = radius * radius, every operation a separately rounded f64
// operation; the bound is inclusive.  A query that is not finite after the transform has no neighbours.  The list of a query is ordered by
// ascending (d2, target buffer index).
//
// Shape.  One lane per query, queries in the order of their cell keys (nn.hip's keys and the pair sort): the lanes of a wave are neighbours
// and walk the same rows.  The index's cell edge comes from the density, not from the radius, so a ball spans one cell or hundreds: the
// lane walks the (y, z) rows of the ball's clamped cell box, culls each row and trims it to the ball's chord (radius_cull.hpp), finds the
// row's key range [row | x0, (row | x1) + 1) in the sorted keys -- a binary search for the start, a galloping one for the end -- and tests
// every candidate of it.  The count kernel and the fill kernel do the SAME walk; the fill writes (buffer index, ordered key of d2) into the
// query's range of the CSR arrays in walk order, which depends on the grid.  The order kernels remove that dependence:
//   short   lists of at most kRadiusSortCap entries.  Workgroup b loads the window of kRadiusSortWindow entries from position
//           b * kRadiusSortPositionsPerBlock into LDS as (list code, d2 key, index) and sorts it with one bitonic network on that triple
//           (quantiles.hip's design).  The list code is monotone along the window, so every entry stays inside its list.  A short list whose
//           HEAD lies in the workgroup's first kRadiusSortPositionsPerBlock positions ends inside the window and is written by this
//           workgroup alone.  A workgroup also READS entries of lists it does not own while their owner may be writing them: what it reads
//           there can be any mixture, it sorts behind or in front of the owned lists as its code says and is never written.
//   long    listed by one lane per query (integer atomics that append to the list, nothing else), their entries compacted and sent through
//           the stable radix sorts: by index, by d2 key, by the list's place in the list of long lists.  The order of that list moves the
//           runs about in scratch and changes nothing that is written.
// No floating-point atomics.  The result is a function of the two clouds, the transform and the radius alone.
//
// Which rows and cells may be skipped.  Everything is done in CELL UNITS of the index's grid: a = (q' - min) / edge, Rc = radius / edge.
// Let S = |ax| + |ay| + |az| + Rc + (largest dim) + 1: every number the cull computes is at most S in magnitude (S >= 1).
//   the predicate   fl is monotone and the terms are not negative, so a neighbour has fl(dx*dx) <= r2 and the like per term, and
//                   (dx*dx + dy*dy + dz*dz)(1 - 2^-51) <= d2 <= r2 <= radius^2 (1 + 2^-53) in the normal range (r2 IS normal: the API checks it; a
//                   term in the subnormal range is off by 2^-1075 absolutely, far below r2 * 2^-53).  fl(p - q') is within 2^-53 relative per
//                   component.  So the real distance |p - q'| <= radius (1 + 2^-49).
//   the cells       a target's cell number is trunc(fl(fl(p - min) / edge)), two roundings of a value below 2^21: a target of cell k has its
//                   real coordinate (p - min) / edge in [k - 2^-30, k + 1 + 2^-30] (the argument of nn.hip).
//   the units       a and Rc carry two roundings each, 2^-52 S at the most; in real cell units the neighbour lies within
//                   Rc* = Rc (1 + 2^-48) of the real centre, which is within 2^-52 S of a per axis.
//   the margin      pad = 2^-22 S, Rp = Rc + pad.  Everything above sums to less than eta = 2^-29 S (S >= 1 covers the cells' 2^-30).
//   the box         per axis |p_k - a_k| <= Rc* + eta < Rp: the cells of [a_k - Rp, a_k + Rp], clamped to the grid; an empty clamp on any axis
//                   ends the query before any search.
//   a row           (iy, iz): let G be the distance from (a_y, a_z) to the rectangle [iy, iy + 1] x [iz, iz + 1] as computed (two
//                   subtractions, two squares, a sum: 2^-51 relative in G^2).  A neighbour in the row has (y, z) within 2^-30 sqrt(2) of that
//                   rectangle, so its real transverse distance T from the centre is at least G - eta, and T <= Rc*: G <= Rc* + eta
//                   <= Rp - pad / 2.  Squares are compared: G^2 <= Rp^2 (1 - pad / (2 Rp))^2, and pad / Rp >= 2^-23 (Rp <= S (1 + 2^-22)), a relative gap
//                   of 2^-24 against roundings of 2^-50.  So a row with G^2 > Rp^2 holds no neighbour.
//   the chord       along x the neighbour has |p_x - a_x| <= sqrt(Rc*^2 - T^2) + eta.  Rp^2 - G^2 - (Rc*^2 - T^2) = (Rp - Rc*)(Rp + Rc*) - (G - T)(G + T)
//                   >= (pad / 2) Rp - eta * 2 Rp >= 0: the real sqrt(Rp^2 - G^2) bounds the chord.  The computed h2 = Rp^2 - G^2 is off by at
//                   most 2^-50 S^2 absolutely, its root by at most 2^-25 S (sqrt(x + e) <= sqrt(x) + sqrt(e)), the root's own rounding by 2^-53 S:
//                   h = sqrt(max(h2, 0)) + pad covers all of it and eta eight times over.  The row's cells are those of [a_x - h, a_x + h].
//   not finite      every comparison of the cull is written so that a NaN (an S that overflows) keeps the row or the whole axis: the cull
//                   can only ever drop what the argument above covers.
// Hence a cell is skipped only when no point of it can satisfy the ROUNDED predicate: the result does not depend on the grid.
//
// Cost.  The row test is a dozen flops per row of the BOX, the searches are two chains of dependent loads per row of the BALL.  A ball that
// spans a whole fine grid tests every row of it; that is accepted, as nn.hip accepts its far query.
#include "positions_device.hpp"
#include "radius_cull.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kQ = pstk::kRadiusQueriesPerBlock;
constexpr uint32_t kCap = pstk::kRadiusSortCap;
constexpr uint32_t kWindow = pstk::kRadiusSortWindow;
constexpr uint32_t kPpb = pstk::kRadiusSortPositionsPerBlock;
constexpr uint32_t kPerLane = kWindow / kBlock;
// LDS of the window kernel: the d2 keys, the indices and the list codes.  28 KiB: five workgroups (20 waves, five per SIMD) share a CU's
// 160 KiB, which is what hides the barrier of every network stage behind the other workgroups' stages (quantiles.hip)
constexpr uint32_t kWindowLds = kWindow * (8 + 4 + 2);
static_assert(kQ == kBlock, "one lane per query");
static_assert((kWindow & (kWindow - 1)) == 0 && kWindow % (2 * kBlock) == 0, "the bitonic network: a power of two, whole pairs per lane");
static_assert(kPpb + kCap - 1 <= kWindow, "a short list that starts in the workgroup's positions ends inside the window");
static_assert(kWindow + 1 < 0xFFFF, "list codes are kept as uint16, 0xFFFF is the padding's");
static_assert(kPerLane <= 32, "the owned positions of a lane are a bit mask");
static_assert(kWindowLds * 5 <= 160 * 1024, "five workgroups per CU");

using Args = pstk::RadiusSearch;
using ull = unsigned long long;

__device__ __forceinline__ void apply(const pstk::NnTransform& t, double& x, double& y, double& z) {  // nn.hip's expression: the same bits
  if (!t.on) return;
  const double a = ((t.m[0] * x + t.m[1] * y) + t.m[2] * z) + t.m[3];
  const double b = ((t.m[4] * x + t.m[5] * y) + t.m[6] * z) + t.m[7];
  const double c = ((t.m[8] * x + t.m[9] * y) + t.m[10] * z) + t.m[11];
  x = a; y = b; z = c;
}

// first position in keys[lo, hi) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const ull* __restrict__ keys, uint32_t lo, uint32_t hi, ull k) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the same from `first` on, for a position that is expected close behind it (m3c2.hip's)
__device__ __forceinline__ uint32_t gallop_bound(const ull* __restrict__ keys, uint32_t first, uint32_t nf, ull k) {
  uint32_t lo = first, hi = first, step = 8;
  while (hi < nf && keys[hi] < k) {
    lo = hi + 1;
    hi = step < nf - hi ? hi + step : nf;
    step <<= 1;
  }
  return lower_bound(keys, lo, hi, k);
}

// ---- count and fill: the same walk ----------------------------------------------------------------------------------------------------------------
// FILL: the neighbours go to indices / d2_keys at [offsets[i], offsets[i + 1]); else their number goes to counts[i]
template <bool FILL>
__global__ __launch_bounds__(kBlock) void radius_walk_kernel(Args p, uint32_t* __restrict__ counts, const ull* __restrict__ offsets, uint32_t* __restrict__ indices,
                                                             ull* __restrict__ d2_keys) {
  const uint64_t s = (uint64_t)blockIdx.x * kQ + threadIdx.x;
  if (s >= p.pos.n) return;
  const uint32_t i = p.query_order[s];
  uint32_t found = 0;
  ull at = 0, end = 0;
  if constexpr (FILL) { at = offsets[i]; end = offsets[i + 1]; }
  const bool walk = FILL ? at < end : p.query_keys[s] != ~0ull;  // (not finite: keyed behind every finite query, no neighbours)
  if (walk) {
    double q[3];
    load_point(Pos{(cgptr_t)p.pos.base, p.pos.stride}, i, q[0], q[1], q[2]);
    apply(p.t, q[0], q[1], q[2]);
    pstk::RadiusBall b;
    if (radius_ball(q, p.radius, p.g.min, p.g.edge, p.g.dim, b)) {
      const uint32_t bx = p.g.bits[0], by = p.g.bits[1];
      const uint32_t nf = p.nf;
#pragma unroll 1
      for (uint32_t iz = b.c0[2]; iz <= b.c1[2]; ++iz) {
#pragma unroll 1
        for (uint32_t iy = b.c0[1]; iy <= b.c1[1]; ++iy) {
          uint32_t x0, x1;
          if (!radius_row_cells(b, iy, iz, p.g.dim[0], x0, x1)) continue;
          const ull row = ((ull)iz << (bx + by)) | ((ull)iy << bx);
          const uint32_t first = lower_bound(p.keys, 0, nf, row | x0);
          const uint32_t last = gallop_bound(p.keys, first, nf, (row | x1) + 1);
          for (uint32_t c = first; c < last; ++c) {
            const double dx = p.xs[c] - q[0], dy = p.ys[c] - q[1], dz = p.zs[c] - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= p.r2) {
              if constexpr (FILL) {
                if (at < end) {  // (the count's walk over again: always true; a write can never leave the query's range)
                  indices[at] = p.target_index[c];
                  d2_keys[at] = ordered(d2);
                  ++at;
                }
              } else {
                ++found;
              }
            }
          }
        }
      }
    }
  }
  if constexpr (!FILL) counts[i] = found;
}

// ---- the order inside the lists -------------------------------------------------------------------------------------------------------------------
// the last list i of [lo, hi) with offsets[i] <= e, given offsets[lo] <= e: the list that holds entry e when hi's offset is beyond it
__device__ __forceinline__ uint32_t list_of(const ull* __restrict__ offsets, uint32_t lo, uint32_t hi, ull e) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void radius_window_kernel(const ull* __restrict__ offsets, uint32_t n, ull total, uint32_t cap, uint32_t* indices,
                                                               const ull* __restrict__ d2_keys, double* __restrict__ distances) {
  __shared__ ull s_key[kWindow];
  __shared__ uint32_t s_idx[kWindow];
  __shared__ uint16_t s_code[kWindow];
  const ull base = (ull)blockIdx.x * kPpb;  // below total (the launcher's grid)
  const ull stop = base + kWindow < total ? base + kWindow : total;
  // the lists of the window's first and last entry bracket every entry's search
  const uint32_t l_first = list_of(offsets, 0, n, base);
  const uint32_t l_last = list_of(offsets, l_first, n, stop - 1);
  // the window: entries by (list code, d2 key, index).  Code 0: the list that began before the window; 1 + the head's position otherwise;
  // 0xFFFF behind the last entry.  The codes ascend along the window.
  uint32_t owned = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPerLane; ++j) {
    const uint32_t w = j * kBlock + threadIdx.x;
    const ull e = base + w;
    uint16_t code = 0xFFFFu;
    ull key = 0;
    uint32_t idx = 0;
    if (e < stop) {
      const uint32_t l = list_of(offsets, l_first, l_last + 1, e);
      const ull head = offsets[l], len = offsets[l + 1] - head;
      code = head < base ? (uint16_t)0 : (uint16_t)(head - base + 1);
      key = d2_keys[e];
      idx = indices[e];
      if (head >= base && head - base < kPpb && len <= cap) owned |= 1u << j;
    }
    s_code[w] = code;
    s_key[w] = key;
    s_idx[w] = idx;
  }
  if (!__syncthreads_or(owned != 0)) return;  // (uniform) nothing but the inside of long lists and of the neighbours' lists
#pragma unroll 1
  for (uint32_t k = 2; k <= kWindow; k <<= 1) {
#pragma unroll 1
    for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
#pragma unroll
      for (uint32_t q = 0; q < kPerLane / 2; ++q) {
        const uint32_t t = q * kBlock + threadIdx.x;               // the t-th pair of this stage
        const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // its lower element: bit j clear
        const uint32_t b = a | j;
        const uint32_t ca = s_code[a], cb = s_code[b];
        const ull ka = s_key[a], kb = s_key[b];
        const uint32_t ia = s_idx[a], ib = s_idx[b];
        const bool a_above_b = ca > cb || (ca == cb && (ka > kb || (ka == kb && ia > ib)));
        const bool differ = ca != cb || ka != kb || ia != ib;
        const bool ascending = (a & k) == 0;
        if (a_above_b == ascending && differ) {
          s_code[a] = (uint16_t)cb; s_code[b] = (uint16_t)ca;
          s_key[a] = kb; s_key[b] = ka;
          s_idx[a] = ib; s_idx[b] = ia;
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kPerLane; ++j) {
    if (!((owned >> j) & 1u)) continue;
    const uint32_t w = j * kBlock + threadIdx.x;
    indices[base + w] = s_idx[w];
    if (distances) distances[base + w] = __builtin_sqrt(decode_ordered(s_key[w]));
  }
}

__global__ __launch_bounds__(kBlock) void radius_list_long_kernel(const ull* __restrict__ offsets, uint32_t n, uint32_t cap, uint32_t* __restrict__ long_list,
                                                                  uint32_t* __restrict__ long_size, uint32_t* long_count) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const ull m = offsets[i + 1] - offsets[i];
  if (m > cap) {
    const uint32_t slot = atomicAdd(long_count, 1u);  // (at most total / (cap + 1) lists can be this long)
    long_list[slot] = i;
    long_size[slot] = (uint32_t)m;  // (total < 2^32 - 16)
  }
}

// One lane per listed entry j: its list is the last place o of long_list with long_offset[o] <= j
__global__ __launch_bounds__(kBlock) void radius_long_compact_kernel(const ull* __restrict__ offsets, const uint32_t* __restrict__ long_list, const ull* __restrict__ long_offset,
                                                                     uint32_t n_long, uint32_t n_listed, const uint32_t* __restrict__ indices,
                                                                     const ull* __restrict__ d2_keys, uint32_t* __restrict__ idx, uint32_t* __restrict__ idx_keys,
                                                                     ull* __restrict__ keys, uint32_t* __restrict__ owner) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_listed) return;
  const uint32_t o = list_of(long_offset, 0, n_long, j);
  const ull src = offsets[long_list[o]] + (j - long_offset[o]);
  const uint32_t v = indices[src];
  idx[j] = v;
  idx_keys[j] = v;
  keys[j] = d2_keys[src];
  owner[j] = o;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void radius_gather_kernel(const T* __restrict__ in, const uint32_t* __restrict__ slots, uint32_t n, T* __restrict__ out) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < n) out[r] = in[slots[r]];
}

__global__ __launch_bounds__(kBlock) void radius_long_scatter_kernel(const ull* __restrict__ offsets, const uint32_t* __restrict__ long_list, const ull* __restrict__ long_offset,
                                                                     uint32_t n_listed, const uint32_t* __restrict__ ranked, const uint32_t* __restrict__ sorted_owner,
                                                                     const uint32_t* __restrict__ idx, const ull* __restrict__ keys, uint32_t* __restrict__ indices,
                                                                     double* __restrict__ distances) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_listed) return;
  const uint32_t slot = ranked[r], o = sorted_owner[r];
  const ull dst = offsets[long_list[o]] + (r - long_offset[o]);  // (sorted by owner: the run of o starts at long_offset[o])
  indices[dst] = idx[slot];
  if (distances) distances[dst] = __builtin_sqrt(decode_ordered(keys[slot]));
}

}  // namespace

namespace pstk {

bool radius_count(const RadiusSearch& a, uint32_t* counts, hipStream_t stream) {
  if (a.pos.n == 0) return true;
  hipLaunchKernelGGL(radius_walk_kernel<false>, dim3(blocks_of(a.pos.n, kQ)), dim3(kBlock), 0, stream, a, counts, (const ull*)nullptr, (uint32_t*)nullptr, (ull*)nullptr);
  return launched();
}

bool radius_fill(const RadiusSearch& a, const unsigned long long* offsets, uint32_t* indices, unsigned long long* d2_keys, hipStream_t stream) {
  if (a.pos.n == 0) return true;
  hipLaunchKernelGGL(radius_walk_kernel<true>, dim3(blocks_of(a.pos.n, kQ)), dim3(kBlock), 0, stream, a, (uint32_t*)nullptr, offsets, indices, d2_keys);
  return launched();
}

bool radius_order_short(const unsigned long long* offsets, uint32_t n, uint64_t total, uint32_t cap, uint32_t* indices, const unsigned long long* d2_keys, double* distances,
                        hipStream_t stream) {
  if (cap == 0 || total == 0 || n == 0) return true;  // every list is listed
  if (cap > kCap) return false;
  hipLaunchKernelGGL(radius_window_kernel, dim3(blocks_of(total, kPpb)), dim3(kBlock), 0, stream, offsets, n, (ull)total, cap, indices, d2_keys, distances);
  return launched();
}

bool radius_list_long(const unsigned long long* offsets, uint32_t n, uint32_t cap, uint32_t* long_list, uint32_t* long_size, uint32_t* long_count, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(radius_list_long_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, offsets, n, cap, long_list, long_size, long_count);
  return launched();
}

bool radius_long_compact(const unsigned long long* offsets, const uint32_t* long_list, const unsigned long long* long_offset, uint32_t n_long, uint32_t n_listed,
                         const uint32_t* indices, const unsigned long long* d2_keys, uint32_t* idx, uint32_t* idx_keys, unsigned long long* keys, uint32_t* owner,
                         hipStream_t stream) {
  hipLaunchKernelGGL(radius_long_compact_kernel, dim3(blocks_of(n_listed, kBlock)), dim3(kBlock), 0, stream, offsets, long_list, long_offset, n_long, n_listed, indices, d2_keys,
                     idx, idx_keys, keys, owner);
  return launched();
}

bool radius_gather_u64(const unsigned long long* keys, const uint32_t* slots, uint32_t n, unsigned long long* out, hipStream_t stream) {
  hipLaunchKernelGGL(radius_gather_kernel<ull>, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, keys, slots, n, out);
  return launched();
}

bool radius_gather_u32(const uint32_t* owner, const uint32_t* slots, uint32_t n, uint32_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(radius_gather_kernel<uint32_t>, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, owner, slots, n, out);
  return launched();
}

bool radius_long_scatter(const unsigned long long* offsets, const uint32_t* long_list, const unsigned long long* long_offset, uint32_t n_listed, const uint32_t* ranked,
                         const uint32_t* sorted_owner, const uint32_t* idx, const unsigned long long* keys, uint32_t* indices, double* distances, hipStream_t stream) {
  hipLaunchKernelGGL(radius_long_scatter_kernel, dim3(blocks_of(n_listed, kBlock)), dim3(kBlock), 0, stream, offsets, long_list, long_offset, n_listed, ranked,
                     sorted_owner, idx, keys, indices, distances);
  return launched();
}

}  // namespace pstk
