// Segment statistics: per-label count, box, centroid, covariance and value statistics (include/pasture_amd.h, "Segment statistics").
//
// Definitions.  A point's value v is its z, or values[i].  A member of segment s = labels[i]: s < S, x, y, z and v finite, a non-zero mask
// byte.  Per segment over its members in ascending buffer index, every sum is the TREE T: the sequence is cut into groups of 256 (the last
// one padded with -0.0, the identity of IEEE addition), a group gives r_l = ((g_l + g_(l+64)) + g_(l+128)) + g_(l+192) for l < 64 and then
// r_l = r_l + r_(l+h) for l < h, h = 32 .. 1; the r_0 of the groups, in order, are the next sequence, until one value is left.  Every
// operation a separately rounded f64 operation.
//
// One path.  key = label of a member, S of every other point; the stable radix sort with the point index as payload, so that a segment's
// run is in buffer-index order; the dense directory by run heads and the suffix minimum (raster.hip's); x, y, z and v gathered into four
// columns in sorted order.  Then the fold: ONE WAVE PER GROUP, at every level.  Level k of a segment holds c_k elements (c_0 = its members)
// in ceil(c_k / 256) groups; a segment of one group is finished by that group's wave, which writes the segment's planes; a segment of more
// writes its partials, contiguous and in group order, and they are its elements of level k + 1.  A lane loads its four elements with four
// coalesced loads, adds them, and takes the six halving steps with cross-lane moves; minima, maxima and the apex ride along (they are
// order-free).  The second pass folds the six products of the deviations from the centroid and the squared value deviation the same way.
// No lane walks a segment, and nothing here is an atomic on a per-segment record.
#include <algorithm>

#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPpb = pstk::kSegmentsPointsPerBlock;
constexpr uint32_t kGroup = pstk::kSegmentGroup;
constexpr uint32_t kGpb = pstk::kSegmentsGroupsPerBlock;
static_assert(kPpb == kBlock, "one point per lane in the key and gather kernels");
static_assert(kGroup == 256 && kGpb * 64 == kBlock, "a wave owns one group: four elements per lane");

using Input = pstk::SegmentInput;
using Planes = pstk::SegmentPlanes;
using Level = pstk::SegmentLevel;
using Fold = pstk::SegmentFold;

__device__ __forceinline__ double canonical_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }
__device__ __forceinline__ double minus_zero() { return __builtin_bit_cast(double, 0x8000000000000000ull); }

// ---- keys, gather ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void segment_key_kernel(Pos pos, uint64_t n, Input in, uint32_t n_segments, uint32_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t label = in.labels[i];
  bool member = label < n_segments && (!in.mask || in.mask[i]);
  if (member) {
    double x, y, z;
    load_point(pos, i, x, y, z);
    const double v = in.values ? in.values[i] : z;
    member = finite(x) && finite(y) && finite(z) && finite(v);
  }
  keys[i] = member ? label : n_segments;
}

__global__ __launch_bounds__(kBlock) void segment_gather_kernel(Pos pos, Input in, const uint32_t* __restrict__ order, const uint32_t* __restrict__ dir, uint32_t n_segments,
                                                                double* __restrict__ xs, double* __restrict__ ys, double* __restrict__ zs, double* __restrict__ vs) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= dir[n_segments]) return;
  const uint32_t i = order[s];
  double x, y, z;
  load_point(pos, i, x, y, z);
  xs[s] = x;
  ys[s] = y;
  zs[s] = z;
  if (vs) vs[s] = in.values[i];  // (without values the value column IS the z column)
}

// ---- per segment: the counts, the empty values, the levels' tables --------------------------------------------------------------------------------
// count[s] = members, groups[s] = ceil(members / 256) (entry S of both: 0, for the scans); the COUNT plane; an empty segment's other planes
__global__ __launch_bounds__(kBlock) void segment_counts_kernel(const uint32_t* __restrict__ dir, uint32_t n_segments, Planes out, uint32_t* __restrict__ apex,
                                                                uint32_t* __restrict__ count, uint32_t* __restrict__ groups) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s > n_segments) return;
  if (s == n_segments) {
    count[s] = 0;
    groups[s] = 0;
    return;
  }
  const uint32_t m = dir[s + 1] - dir[s];
  count[s] = m;
  groups[s] = (m + kGroup - 1) / kGroup;
  if (out.count) out.count[s] = (double)m;
  if (m) return;
  const size_t S = n_segments;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (out.min) out.min[c * S + s] = canonical_nan();
    if (out.max) out.max[c * S + s] = canonical_nan();
    if (out.centroid) out.centroid[c * S + s] = canonical_nan();
  }
  if (out.covariance) {
#pragma unroll
    for (int c = 0; c < 6; ++c) out.covariance[c * S + s] = canonical_nan();
  }
  if (out.value_min) out.value_min[s] = canonical_nan();
  if (out.value_max) out.value_max[s] = canonical_nan();
  if (out.value_mean) out.value_mean[s] = canonical_nan();
  if (out.value_variance) out.value_variance[s] = canonical_nan();
  if (apex) apex[s] = 0xFFFFFFFFu;
}

// the next level: a segment of more than one group goes on with its partials, every other one is finished
__global__ __launch_bounds__(kBlock) void segment_next_level_kernel(const uint32_t* __restrict__ groups, uint32_t n_segments, uint32_t* __restrict__ next_count,
                                                                    uint32_t* __restrict__ next_groups) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s > n_segments) return;
  const uint32_t g = s < n_segments ? groups[s] : 0;
  const uint32_t c = g > 1 ? g : 0;
  next_count[s] = c;
  next_groups[s] = (c + kGroup - 1) / kGroup;
}

// ---- the fold -----------------------------------------------------------------------------------------------------------------------------------
// the group's r_0 in every lane: the lane's own four elements are added already
__device__ __forceinline__ double halve(double r) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) r = r + shfl_xor_any(r, h);  // lane l < h: r_l + r_(l+h); addition commutes, so every lane holds the same
  return r;
}

template <bool kMin>
__device__ __forceinline__ unsigned long long halve_key(unsigned long long k) {
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const unsigned long long o = shfl_xor_any(k, h);
    k = kMin ? (o < k ? o : k) : (o > k ? o : k);
  }
  return k;
}

// One wave per group.  kProducts: the elements of the sums are computed from the columns and the means (the second pass's first level).
template <bool kProducts>
__global__ __launch_bounds__(kBlock) void segment_fold_kernel(Fold f) {
  // (readfirstlane: the wave number is the same in every lane, and saying so keeps the search below on scalar loads)
  const uint64_t g = (uint64_t)blockIdx.x * kGpb + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (g >= f.level.n_groups) return;
  const uint32_t lane = threadIdx.x & 63;
  const Level& lv = f.level;
  // the segment of group g: the last s with group_offset[s] <= g (group_offset[0] = 0, group_offset[S] = n_groups > g)
  uint32_t lo = 0, hi = f.n_segments;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (lv.group_offset[mid] <= g) lo = mid;
    else hi = mid;
  }
  const uint32_t s = lo;
  const uint32_t c = lv.count[s];
  const uint32_t j = (uint32_t)(g - lv.group_offset[s]);  // the group within the segment: j * 256 < c
  const bool last_level = c <= kGroup;                    // the segment's only group: its result
  const uint64_t first = lv.element_offset[s] + (uint64_t)j * kGroup;
  const uint32_t len = c - j * kGroup < kGroup ? c - j * kGroup : kGroup;
  const uint64_t partial_at = last_level ? 0 : lv.partial_offset[s] + j;
  const double m = (double)(f.dir[s + 1] - f.dir[s]);
  bool in[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) in[q] = lane + 64 * q < len;

  if (kProducts) {
    double d[4][4] = {};  // [channel x y z v][element]
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (!f.column[ch]) continue;
      const double mean = f.mean[ch][s];
#pragma unroll
      for (int q = 0; q < 4; ++q) d[ch][q] = in[q] ? f.column[ch][first + lane + 64 * q] - mean : 0.0;
    }
    // xx xy xz yy yz zz, then the value's
    constexpr int kA[7] = {0, 0, 0, 1, 1, 2, 3}, kB[7] = {0, 1, 2, 1, 2, 2, 3};
#pragma unroll
    for (int ch = 0; ch < 7; ++ch) {
      if (!f.sum_result[ch]) continue;
      double e[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) e[q] = in[q] ? d[kA[ch]][q] * d[kB[ch]][q] : minus_zero();
      const double r = halve(((e[0] + e[1]) + e[2]) + e[3]);
      if (lane == 0) {
        if (last_level) f.sum_result[ch][s] = r / m;
        else f.sum_out[ch][partial_at] = r;
      }
    }
    return;
  }

#pragma unroll
  for (int ch = 0; ch < 7; ++ch) {
    if (!f.sum_in[ch]) continue;
    double e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = in[q] ? f.sum_in[ch][first + lane + 64 * q] : minus_zero();
    const double r = halve(((e[0] + e[1]) + e[2]) + e[3]);
    if (lane == 0) {
      if (last_level) f.sum_result[ch][s] = r / m;
      else f.sum_out[ch][partial_at] = r;
    }
  }
  // minima and maxima of x y z v by the ordered key (a member is finite: its key is neither zero nor all ones, the two identities)
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    if (f.min_in[ch]) {
      unsigned long long k = ~0ull;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long o = in[q] ? ordered(f.min_in[ch][first + lane + 64 * q]) : ~0ull;
        k = o < k ? o : k;
      }
      k = halve_key<true>(k);
      if (lane == 0) {
        if (!last_level) f.min_out[ch][partial_at] = decode_ordered(k);
        else if (f.min_result[ch]) f.min_result[ch][s] = decode_ordered(k);
      }
    }
    if (f.max_in[ch]) {
      unsigned long long k = 0ull;
      uint32_t at = 0xFFFFFFFFu;  // the apex: the lowest index among the elements that carry the largest key
      const bool with_apex = ch == 3 && f.apex_in;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long o = in[q] ? ordered(f.max_in[ch][first + lane + 64 * q]) : 0ull;
        const uint32_t oat = with_apex && in[q] ? f.apex_in[first + lane + 64 * q] : 0xFFFFFFFFu;
        const bool better = o > k || (o == k && oat < at);
        k = better ? o : k;
        at = better ? oat : at;
      }
      if (with_apex) {
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
          const unsigned long long o = shfl_xor_any(k, h);
          const uint32_t oat = shfl_xor_any(at, h);
          const bool better = o > k || (o == k && oat < at);
          k = better ? o : k;
          at = better ? oat : at;
        }
      } else {
        k = halve_key<false>(k);
      }
      if (lane == 0) {
        if (!last_level) {
          f.max_out[ch][partial_at] = decode_ordered(k);
          if (with_apex) f.apex_out[partial_at] = at;
        } else {
          if (f.max_result[ch]) f.max_result[ch][s] = decode_ordered(k);
          if (with_apex && f.apex_result) f.apex_result[s] = at;
        }
      }
    }
  }
}

}  // namespace

namespace pstk {

bool segment_keys(const Positions& pos, const SegmentInput& in, uint32_t n_segments, uint32_t* keys, hipStream_t stream) {
  hipLaunchKernelGGL(segment_key_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, in, n_segments, keys);
  return launched();
}

bool segment_gather(const Positions& pos, const SegmentInput& in, const uint32_t* order, const uint32_t* dir, uint32_t n_segments, double* xs, double* ys, double* zs,
                    double* vs, hipStream_t stream) {
  hipLaunchKernelGGL(segment_gather_kernel, dim3(blocks_of(pos.n, kPpb)), dim3(kBlock), 0, stream, pos_of(pos), in, order, dir, n_segments, xs, ys, zs, vs);
  return launched();
}

bool segment_counts(const uint32_t* dir, uint32_t n_segments, const SegmentPlanes& out, uint32_t* apex, uint32_t* count, uint32_t* groups, hipStream_t stream) {
  hipLaunchKernelGGL(segment_counts_kernel, dim3(blocks_of((uint64_t)n_segments + 1, kBlock)), dim3(kBlock), 0, stream, dir, n_segments, out, apex, count, groups);
  return launched();
}

bool segment_next_level(const uint32_t* groups, uint32_t n_segments, uint32_t* next_count, uint32_t* next_groups, hipStream_t stream) {
  hipLaunchKernelGGL(segment_next_level_kernel, dim3(blocks_of((uint64_t)n_segments + 1, kBlock)), dim3(kBlock), 0, stream, groups, n_segments, next_count, next_groups);
  return launched();
}

bool segment_fold(const SegmentFold& f, bool products, hipStream_t stream) {
  if (f.level.n_groups == 0) return true;
  if (f.level.n_groups > (uint64_t)0x7FFFFFFF * kGpb) return false;  // (never: fewer groups than points + segments)
  const dim3 grid(blocks_of(f.level.n_groups, kGpb));
  if (products) hipLaunchKernelGGL(segment_fold_kernel<true>, grid, dim3(kBlock), 0, stream, f);
  else hipLaunchKernelGGL(segment_fold_kernel<false>, grid, dim3(kBlock), 0, stream, f);
  return launched();
}

}  // namespace pstk
