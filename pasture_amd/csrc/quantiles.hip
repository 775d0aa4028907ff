// Group order statistics: quantiles and counts above a threshold per cell or per segment (include/pasture_amd.h, "Quantiles").
//
// Definitions.  s_0 .. s_(m-1) are a group's member values in ascending order of the ordered() key.  Per probability p: h = (double)(m - 1) * p,
// lo = (uint32)floor(h), g = h - (double)lo, and the method picks s_lo, s_(lo+1) or s_lo + g * (s_(lo+1) - s_lo); per threshold t: the number of
// members with v > t compared as doubles.  Every operation a separately rounded f64 operation.
//
// The front end is raster.hip's and segments.hip's: keys, the stable radix sort with the point index as payload, the dense directory, the value
// column gathered into sorted order -- every group is a contiguous run of `values`, and `group_of[s]` (the sorted keys) names the group of
// sorted position s.  What is new is the order INSIDE the runs:
//   small   m <= kQuantilesCap.  Workgroup b loads the window of kQuantilesWindow sorted positions from b * kQuantilesPointsPerBlock into LDS
//           as (group, ordered key) and sorts it with one bitonic network on that pair.  The window is sorted by group already, so every
//           element stays inside its run and the network orders all runs of the window at once: a group of 10 shares the workgroup with 150
//           others.  A small group whose HEAD lies in the first kQuantilesPointsPerBlock positions ends inside the window
//           (kQuantilesPointsPerBlock + kQuantilesCap - 1 <= kQuantilesWindow) and belongs to this workgroup; the heads are compacted in order,
//           and thread t takes (plane, t-th group): the ranks are read from LDS and a plane's results leave in ascending group order.  The
//           sorted values never return to memory, and no lane walks a run.
//   large   m > kQuantilesCap, listed by the per-group kernel.  Their members are compacted as (ordered key, slot), sorted by key
//           (sort_pairs_u64), then stably by the group's place in the list (sort_pairs_u32): rank r of listed group i is entry offset[i] + r.
//           One wave per group, lane = plane.  The order of the list moves the runs about in that scratch and nothing else.
// The result is a function of every group's multiset of keys alone: both paths read ranks of the one ascending order.
#include <algorithm>

#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPpb = pstk::kQuantilesPointsPerBlock;
constexpr uint32_t kCap = pstk::kQuantilesCap;
constexpr uint32_t kWindow = pstk::kQuantilesWindow;
constexpr uint32_t kPerLane = kWindow / kBlock;
constexpr uint32_t kRounds = kPpb / kBlock;
// LDS of the window kernel: the keys, the groups, the heads' list and the waves' head counts.  27 KiB and a bit: five workgroups (20 waves,
// five per SIMD) share a CU's 160 KiB, which is what hides the barrier of every network stage behind the other workgroups' stages
constexpr uint32_t kWindowLds = kWindow * (8 + 4) + kPpb * 2 + (kRounds * (kBlock / 64) + 1) * 4;
static_assert((kWindow & (kWindow - 1)) == 0 && kWindow % (2 * kBlock) == 0, "the bitonic network: a power of two, whole pairs per lane");
static_assert(kPpb % kBlock == 0 && kPpb + kCap - 1 <= kWindow, "a small group that starts in the workgroup's positions ends inside the window");
static_assert(kWindow <= 65536, "window positions are kept as uint16");
static_assert(kWindowLds * 5 <= 160 * 1024, "five workgroups per CU");

using Request = pstk::QuantileRequest;

__device__ __forceinline__ double canonical_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }

// the quantile of probability p over m >= 1 ascending keys read through key_at(rank)
template <typename KeyAt>
__device__ __forceinline__ double quantile_of(uint32_t m, double p, uint32_t method, KeyAt key_at) {
  const double h = (double)(m - 1) * p;  // <= m - 1: the exact product is at most a representable number
  const uint32_t lo = (uint32_t)__builtin_floor(h);
  const double g = h - (double)lo;
  const double a = decode_ordered(key_at(lo));
  if (g == 0.0 || method == pstk::QM_LOWER) return a;
  const double b = decode_ordered(key_at(lo + 1));  // g > 0: h is not an integer, so h < m - 1 and lo + 1 <= m - 1
  if (method == pstk::QM_HIGHER) return b;
  return a + g * (b - a);
}

// the members above t.  `v > t` as doubles is monotone along the ordered() order: that order is the numeric order with -0.0 placed directly
// below +0.0, and the two zeros compare equal to each other and alike to every t -- so the predicate is false on a prefix of the run and true
// on the rest, and the first true rank is found by bisection.
template <typename KeyAt>
__device__ __forceinline__ double above_of(uint32_t m, double t, KeyAt key_at) {
  uint32_t lo = 0, hi = m;  // the first rank with v > t is in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (decode_ordered(key_at(mid)) > t) hi = mid;
    else lo = mid + 1;
  }
  return (double)(m - lo);
}

template <typename KeyAt>
__device__ __forceinline__ double plane_of(const Request& rq, uint32_t plane, uint32_t m, KeyAt key_at) {
  return plane < rq.n_probs ? quantile_of(m, rq.param[plane], rq.method, key_at) : above_of(m, rq.param[plane], key_at);
}

// ---- per group: the COUNT plane, an empty group's planes, the list of the large ones ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void quantile_groups_kernel(const uint32_t* __restrict__ dir, uint32_t n_groups, uint32_t cap, Request rq, double* __restrict__ out,
                                                                 uint32_t* __restrict__ heavy_list, uint32_t* __restrict__ heavy_size, uint32_t* heavy_count) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_groups) return;
  const uint32_t m = dir[c + 1] - dir[c];
  out[c] = (double)m;
  if (m == 0) {
    const uint32_t planes = rq.n_probs + rq.n_thresholds;
    for (uint32_t p = 0; p < planes; ++p) out[(size_t)(1 + p) * n_groups + c] = p < rq.n_probs ? canonical_nan() : 0.0;
  } else if (m > cap) {
    const uint32_t slot = atomicAdd(heavy_count, 1u);  // (at most heavy_capacity(n, n_groups, cap) groups can be this large)
    heavy_list[slot] = c;
    heavy_size[slot] = m;
  }
}

// ---- small groups: the window in LDS ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void quantile_window_kernel(const double* __restrict__ values, const uint32_t* __restrict__ group_of, const uint32_t* __restrict__ dir,
                                                                 uint32_t n_groups, uint32_t cap, Request rq, double* __restrict__ out) {
  __shared__ unsigned long long s_key[kWindow];
  __shared__ uint32_t s_group[kWindow];
  __shared__ uint16_t s_head[kPpb];
  __shared__ uint32_t s_count[kRounds * (kBlock / 64) + 1];
  const uint32_t members = dir[n_groups];
  const uint32_t base = blockIdx.x * kPpb;  // below n < 2^32 - 16 (the launcher's grid)
  if (base >= members) return;              // (uniform) no member's head here
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // the window: members by (group, key); everything behind the last member sorts behind them and is never read
#pragma unroll
  for (uint32_t j = 0; j < kPerLane; ++j) {
    const uint32_t w = j * kBlock + threadIdx.x;
    const uint64_t s = (uint64_t)base + w;
    const bool is_member = s < members;
    s_group[w] = is_member ? group_of[s] : 0xFFFFFFFFu;
    s_key[w] = is_member ? ordered(values[s]) : 0ull;
  }
  // the heads of this workgroup's small groups, compacted in ascending order: ballots, then the waves' counts
  uint32_t before[kRounds];
  bool owned[kRounds];
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t w = r * kBlock + threadIdx.x;
    const uint32_t s = base + w;  // base + w < base + kPpb: no wrap below 2^32 (n < 2^32 - 16 and base < n)
    bool head = false;
    if (s < members) {
      const uint32_t c = group_of[s];
      head = (s == 0 || group_of[s - 1] != c) && dir[c + 1] - s <= cap;  // (a head: dir[c] == s)
    }
    const unsigned long long ballot = __ballot(head);
    owned[r] = head;
    before[r] = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) s_count[r * (kBlock / 64) + wave] = (uint32_t)__popcll(ballot);
  }
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    uint32_t at = 0;
#pragma unroll
    for (uint32_t q = 0; q < kRounds * (kBlock / 64); ++q) {
      const uint32_t cnt = s_count[q];
      if (q < r * (kBlock / 64) + wave) at += cnt;
      if (r == 0) total += cnt;
    }
    if (owned[r]) s_head[at + before[r]] = (uint16_t)(r * kBlock + threadIdx.x);
  }
  if (total == 0) return;  // (uniform) nothing but the inside of large groups
  // the bitonic network on (group, key); every stage ends at a barrier
#pragma unroll 1
  for (uint32_t k = 2; k <= kWindow; k <<= 1) {
#pragma unroll 1
    for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
#pragma unroll
      for (uint32_t q = 0; q < kPerLane / 2; ++q) {
        const uint32_t t = q * kBlock + threadIdx.x;          // the t-th pair of this stage
        const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // its lower element: bit j clear
        const uint32_t b = a | j;
        const uint32_t ga = s_group[a], gb = s_group[b];
        const unsigned long long ka = s_key[a], kb = s_key[b];
        const bool a_above_b = ga > gb || (ga == gb && ka > kb);
        const bool ascending = (a & k) == 0;
        if (a_above_b == ascending && (ga != gb || ka != kb)) {
          s_group[a] = gb; s_group[b] = ga;
          s_key[a] = kb; s_key[b] = ka;
        }
      }
      __syncthreads();
    }
  }
  // thread t: (plane, t-th group), plane-major, so that a plane's results leave in ascending group order
  const uint32_t planes = rq.n_probs + rq.n_thresholds;
  for (uint32_t idx = threadIdx.x; idx < total * planes; idx += kBlock) {
    const uint32_t plane = idx / total, at = s_head[idx - plane * total];
    const uint32_t c = s_group[at];                  // (group-major order: the run's first slot still holds the run's group)
    const uint32_t m = dir[c + 1] - (base + at);
    const unsigned long long* run = s_key + at;       // at + m <= kPpb - 1 + cap <= kWindow
    out[(size_t)(1 + plane) * n_groups + c] = plane_of(rq, plane, m, [run](uint32_t r) { return run[r]; });
  }
}

// ---- large groups --------------------------------------------------------------------------------------------------------------------------------
// One lane per listed member j: its group is the last place i of the list with offset[i] <= j (offset[0] = 0, offset[heavy] = n_listed > j).
// keys[j] = the key of the run's (j - offset[i])-th value, slots[j] = j, owner[j] = i
__global__ __launch_bounds__(kBlock) void quantile_compact_kernel(const double* __restrict__ values, const uint32_t* __restrict__ dir, const uint32_t* __restrict__ heavy_list,
                                                                  const unsigned long long* __restrict__ heavy_offset, uint32_t heavy, uint32_t n_listed,
                                                                  unsigned long long* __restrict__ keys, uint32_t* __restrict__ slots, uint32_t* __restrict__ owner) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_listed) return;
  uint32_t lo = 0, hi = heavy;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (heavy_offset[mid] <= j) lo = mid;
    else hi = mid;
  }
  keys[j] = ordered(values[dir[heavy_list[lo]] + (j - (uint32_t)heavy_offset[lo])]);
  slots[j] = j;
  owner[j] = lo;
}

__global__ __launch_bounds__(kBlock) void quantile_owner_gather_kernel(const uint32_t* __restrict__ owner, const uint32_t* __restrict__ slots, uint32_t n, uint32_t* __restrict__ keys) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < n) keys[r] = owner[slots[r]];
}

// One wave per listed group, lane = plane.  ranked[offset + r] = the slot of the run's r-th smallest; slot - offset = its place in the run.
__global__ __launch_bounds__(kBlock) void quantile_heavy_select_kernel(const double* __restrict__ values, const uint32_t* __restrict__ dir, uint32_t n_groups,
                                                                       const uint32_t* __restrict__ heavy_list, const unsigned long long* __restrict__ heavy_offset,
                                                                       uint32_t heavy, const uint32_t* __restrict__ ranked, Request rq, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t plane = threadIdx.x & 63;
  if (i >= heavy || plane >= rq.n_probs + rq.n_thresholds) return;
  const uint32_t c = heavy_list[i];
  const uint32_t first = dir[c], m = dir[c + 1] - first;
  const uint32_t offset = (uint32_t)heavy_offset[i];
  const uint32_t* rank = ranked + offset;
  const double* run = values + first;
  out[(size_t)(1 + plane) * n_groups + c] = plane_of(rq, plane, m, [=](uint32_t r) { return ordered(run[rank[r] - offset]); });
}

}  // namespace

namespace pstk {

size_t quantile_heavy_capacity(uint64_t n, uint64_t n_groups, uint32_t cap) { return (size_t)std::min<uint64_t>(n / ((uint64_t)cap + 1), n_groups) + 1; }

bool quantile_groups(const uint32_t* dir, uint32_t n_groups, uint32_t cap, const QuantileRequest& rq, double* out, uint32_t* heavy_list, uint32_t* heavy_size,
                     uint32_t* heavy_count, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_groups_kernel, dim3(blocks_of(n_groups, kBlock)), dim3(kBlock), 0, stream, dir, n_groups, cap, rq, out, heavy_list, heavy_size, heavy_count);
  return launched();
}

bool quantile_small_groups(const double* sorted_values, const uint32_t* sorted_keys, const uint32_t* dir, uint32_t n, uint32_t n_groups, uint32_t cap,
                           const QuantileRequest& rq, double* out, hipStream_t stream) {
  if (cap == 0 || n == 0) return true;  // every group is listed
  if (cap > kCap) return false;
  hipLaunchKernelGGL(quantile_window_kernel, dim3(blocks_of(n, kPpb)), dim3(kBlock), 0, stream, sorted_values, sorted_keys, dir, n_groups, cap, rq, out);
  return launched();
}

bool quantile_heavy_compact(const double* sorted_values, const uint32_t* dir, const uint32_t* heavy_list, const unsigned long long* heavy_offset, uint32_t heavy,
                            uint32_t n_listed, unsigned long long* keys, uint32_t* slots, uint32_t* owner, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_compact_kernel, dim3(blocks_of(n_listed, kBlock)), dim3(kBlock), 0, stream, sorted_values, dir, heavy_list, heavy_offset, heavy, n_listed, keys,
                     slots, owner);
  return launched();
}

bool quantile_owner_gather(const uint32_t* owner, const uint32_t* slots, uint32_t n, uint32_t* keys, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_owner_gather_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, owner, slots, n, keys);
  return launched();
}

bool quantile_heavy_select(const double* sorted_values, const uint32_t* dir, uint32_t n_groups, const uint32_t* heavy_list, const unsigned long long* heavy_offset,
                           uint32_t heavy, const uint32_t* ranked, const QuantileRequest& rq, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_heavy_select_kernel, dim3(blocks_of(heavy, kBlock / 64)), dim3(kBlock), 0, stream, sorted_values, dir, n_groups, heavy_list, heavy_offset, heavy,
                     ranked, rq, out);
  return launched();
}

}  // namespace pstk
