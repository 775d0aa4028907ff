// Neighbour distances and outlier criteria over the neighbour lists of the kNN search (normals.hip writes them: uint32 [n][k], ascending distance,
// 0xFFFFFFFF where the cloud has fewer than k points).  Definitions (include/pasture_amd.h, "kNN search and outlier removal"):
//   distance of slot t of query q: dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z (neighbour minus query), sqrt((dx*dx + dy*dy) + dz*dz), every
//   operation a separately rounded f64 operation (-ffp-contract=off); a padded slot has distance +inf
//   statistical: dbar = (d[1] + d[2] + ... + d[mean_k]) / (double)mean_k, summed left to right; mean and standard deviation (two passes) over the
//   finite dbar; keep = dbar finite and dbar <= mean + stddev_mult * stddev
//   radius: keep = d[min_neighbours] <= radius (a padded slot or a NaN compares false)
//
// The distance kernels map the lists flat: a workgroup owns kOutlierPointsPerBlock consecutive points, that is points * k consecutive list elements,
// and walks them kBlock at a time -- element e = q * k + t is read by thread e mod kBlock of its pass, so the index reads (and the distance writes of
// knn_search) are fully coalesced; the query's position is a cached broadcast, the neighbour's the one random 24-byte gather.  For the statistical
// criterion the distances go to an LDS tile (rows padded to an odd number of doubles) and one lane per point sums its row in slot order.
//
// The reductions have a fixed shape: block b of the partial kernels owns points [b * kOutlierReducePoints, ...), a thread adds its four values
// (stride kBlock) in order, the wave folds them in a fixed xor tree, the four waves' sums are added in wave order; ONE workgroup then adds the
// block partials -- thread t the contiguous run [t * c, (t + 1) * c), c = ceil(blocks / kOutlierReduceBlock), in block order, then the same tree.
// Nothing depends on anything but n: two calls on one cloud give the same bits.  No floating-point atomics; the kept count is an integer atomic
// per wave of the mask kernels.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kOutlierPointsPerBlock;
constexpr uint32_t kRP = pstk::kOutlierReducePoints;
constexpr uint32_t kRB = pstk::kOutlierReduceBlock;
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;
static_assert(kRB == kBlock && kRP % kBlock == 0 && kP <= kBlock, "the reduction kernels are written for one kBlock workgroup");

__device__ __forceinline__ double slot_distance(const Pos& pos, uint64_t q, uint32_t j) {
  if (j == kNoIndex) return kInf;
  double qx, qy, qz, px, py, pz;
  load_point(pos, q, qx, qy, qz);
  load_point(pos, j, px, py, pz);
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  return __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
}

// the device-side result record of one call (64 bytes)
struct Record { double mean, stddev, threshold, m; unsigned long long kept, finite_count; double sum, pad; };

// ---- distances ------------------------------------------------------------------------------------------------------------------------------
// STAT = false: dist[e] for every list element.  STAT = true: slots 1 .. mean_k into the LDS tile, then dbar[q] by one lane per point.
template <bool STAT>
__global__ __launch_bounds__(kBlock) void outlier_distance_kernel(Pos pos, uint64_t n, uint32_t k, uint32_t mean_k, const uint32_t* __restrict__ knn,
                                                                  double* __restrict__ out) {
  extern __shared__ double tile[];  // STAT: kP rows of (k | 1) doubles
  const uint64_t q0 = (uint64_t)blockIdx.x * kP;
  const uint32_t points = (uint32_t)(n - q0 < kP ? n - q0 : kP);
  const uint32_t elements = points * k, row = k | 1u;
  const uint64_t e0 = q0 * k;
  for (uint32_t l = threadIdx.x; l < elements; l += kBlock) {
    const uint32_t p = l / k, t = l - p * k;
    if constexpr (STAT) {
      if (t >= 1 && t <= mean_k) tile[p * row + t] = slot_distance(pos, q0 + p, knn[e0 + l]);
    } else {
      out[e0 + l] = slot_distance(pos, q0 + p, knn[e0 + l]);
    }
  }
  if constexpr (STAT) {
    __syncthreads();
    if (threadIdx.x < points) {
      const double* r = tile + threadIdx.x * row;
      double s = r[1];
      for (uint32_t t = 2; t <= mean_k; ++t) s = s + r[t];
      out[q0 + threadIdx.x] = s / (double)mean_k;
    }
  }
}

// radius: one lane per point, one list element and one gather each
__global__ __launch_bounds__(kBlock) void outlier_radius_kernel(Pos pos, uint64_t n, uint32_t k, uint32_t slot, double radius, const uint32_t* __restrict__ knn,
                                                                uint8_t* __restrict__ mask, Record* __restrict__ rec) {
  const uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool keep = false;
  if (q < n) {
    keep = slot_distance(pos, q, knn[q * k + slot]) <= radius;
    mask[q] = keep ? 1 : 0;
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(keep));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rec->kept, c);
}

// ---- fixed-shape sums -------------------------------------------------------------------------------------------------------------------------
// wave: xor tree; block: the waves' sums in wave order.  The result is valid in thread 0.
__device__ __forceinline__ void block_sum(double& v, unsigned long long& c, double* sv, unsigned long long* sc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v = v + shfl_xor_any(v, off);
    c = c + shfl_xor_any(c, off);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sv[wave] = v; sc[wave] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = sv[0]; c = sc[0];
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) { v = v + sv[w]; c = c + sc[w]; }
  }
}

// PASS 0: sum and count of the finite dbar.  PASS 1: sum of (dbar - mean)^2 over them.
template <int PASS>
__global__ __launch_bounds__(kBlock) void outlier_partial_kernel(const double* __restrict__ dbar, uint64_t n, const Record* __restrict__ rec, double* __restrict__ psum,
                                                                 unsigned long long* __restrict__ pcount) {
  __shared__ double sv[kBlock / 64];
  __shared__ unsigned long long sc[kBlock / 64];
  const double mean = PASS == 1 ? rec->mean : 0.0;
  const uint64_t first = (uint64_t)blockIdx.x * kRP;
  double v = 0.0;
  unsigned long long c = 0;
#pragma unroll
  for (uint32_t j = 0; j < kRP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i < n) {
      const double d = dbar[i];
      if (finite(d)) {
        if constexpr (PASS == 0) { v = v + d; }
        else { const double dev = d - mean; v = v + dev * dev; }
        c += 1;
      }
    }
  }
  block_sum(v, c, sv, sc);
  if (threadIdx.x == 0) { psum[blockIdx.x] = v; pcount[blockIdx.x] = c; }
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void outlier_final_kernel(const double* __restrict__ psum, const unsigned long long* __restrict__ pcount, uint64_t blocks,
                                                               double stddev_mult, Record* __restrict__ rec) {
  __shared__ double sv[kBlock / 64];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t per = (blocks + kRB - 1) / kRB, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double v = 0.0;
  unsigned long long c = 0;
  for (uint64_t b = b0; b < b1; ++b) { v = v + psum[b]; c = c + pcount[b]; }
  block_sum(v, c, sv, sc);
  if (threadIdx.x != 0) return;
  if constexpr (PASS == 0) {
    rec->sum = v;
    rec->finite_count = c;
    rec->m = (double)c;
    rec->mean = v / (double)c;  // no finite dbar: 0 / 0, and no point is kept
    rec->kept = 0;
  } else {
    const unsigned long long m = rec->finite_count;
    rec->stddev = m < 2 ? 0.0 : __builtin_sqrt(v / (double)(m - 1));
    const double scaled = stddev_mult * rec->stddev;
    rec->threshold = rec->mean + scaled;
  }
}

__global__ __launch_bounds__(kBlock) void outlier_mask_kernel(const double* __restrict__ dbar, uint64_t n, uint8_t* __restrict__ mask, Record* __restrict__ rec) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const double thr = rec->threshold;
  bool keep = false;
  if (i < n) {
    const double d = dbar[i];
    keep = finite(d) && d <= thr;
    mask[i] = keep ? 1 : 0;
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(keep));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&rec->kept, c);
}

}  // namespace

namespace pstk {

size_t outlier_record_bytes() { return sizeof(Record); }
size_t outlier_partials_bytes(uint64_t n) { return (size_t)blocks_of(n, kRP) * 16; }

bool outlier_distances(const Positions& pos, uint32_t k, const uint32_t* knn_dev, double* dist_dev, hipStream_t stream) {
  if (pos.n == 0) return true;
  hipLaunchKernelGGL(outlier_distance_kernel<false>, dim3(blocks_of(pos.n, kP)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, k, 0u, knn_dev, dist_dev);
  return launched();
}

bool outlier_mean_distances(const Positions& pos, uint32_t k, uint32_t mean_k, const uint32_t* knn_dev, double* dbar_dev, hipStream_t stream) {
  if (pos.n == 0) return true;
  const size_t lds = (size_t)kP * (k | 1u) * sizeof(double);  // at most 64 * 65 * 8 = 33 280 bytes
  hipLaunchKernelGGL(outlier_distance_kernel<true>, dim3(blocks_of(pos.n, kP)), dim3(kBlock), lds, stream, pos_of(pos), pos.n, k, mean_k, knn_dev, dbar_dev);
  return launched();
}

bool outlier_statistics_and_mask(const double* dbar_dev, uint64_t n, double stddev_mult, void* partials, void* record, uint8_t* mask_dev, hipStream_t stream) {
  const unsigned blocks = blocks_of(n, kRP);
  double* psum = (double*)partials;
  unsigned long long* pcount = (unsigned long long*)(psum + blocks);
  Record* rec = (Record*)record;
  hipLaunchKernelGGL(outlier_partial_kernel<0>, dim3(blocks), dim3(kBlock), 0, stream, dbar_dev, n, (const Record*)rec, psum, pcount);
  hipLaunchKernelGGL(outlier_final_kernel<0>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, stddev_mult, rec);
  hipLaunchKernelGGL(outlier_partial_kernel<1>, dim3(blocks), dim3(kBlock), 0, stream, dbar_dev, n, (const Record*)rec, psum, pcount);
  hipLaunchKernelGGL(outlier_final_kernel<1>, dim3(1), dim3(kBlock), 0, stream, (const double*)psum, (const unsigned long long*)pcount, (uint64_t)blocks, stddev_mult, rec);
  hipLaunchKernelGGL(outlier_mask_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, dbar_dev, n, mask_dev, rec);
  return launched();
}

bool outlier_radius_mask(const Positions& pos, uint32_t k, uint32_t slot, double radius, const uint32_t* knn_dev, void* record, uint8_t* mask_dev,
                         hipStream_t stream) {
  if (hipMemsetAsync(record, 0, sizeof(Record), stream) != hipSuccess) return false;
  hipLaunchKernelGGL(outlier_radius_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, k, slot, radius, knn_dev, mask_dev,
                     (Record*)record);
  return launched();
}

}  // namespace pstk
