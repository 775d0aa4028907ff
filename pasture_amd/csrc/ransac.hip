// RANSAC plane / line segmentation: hypothesis table, scoring, arg-max, inlier mask and ordered inlier indices.
// Reference: pasture-algorithms/src/segmentation.rs:31-44 (distances), :47-94 (hypotheses), :96-370 (ransac_{plane,line}_{serial,par}).
//
// Contract (every operation a separately rounded f64 operation, in this order; the library is compiled with -ffp-contract=off):
//   plane  (i1, i2, i3): v1 = p2 - p1, v2 = p3 - p1, n = v1 x v2, d = -((n.x*p1.x + n.y*p1.y) + n.z*p1.z); model (a, b, c, d) = (n, d)
//          inlier: |((a*x + b*y) + c*z) + d| / sqrt((a*a + b*b) + c*c) < thr
//   line   (i1, i2): first = p1, second = p2; dv = second - first, w = first - p, cr = dv x w
//          inlier: sqrt((cr.x^2 + cr.y^2) + cr.z^2) / sqrt((dv.x^2 + dv.y^2) + dv.z^2) < thr
//   cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
//
// The guarded fast path.  Write num for the rounded numerator, e for the rounded denominator, q = fl(num / e) for what the reference compares
// with thr, u = 2^-53.  The record holds t = fl(thr * e), lo = fl(t * (1 - 2^-40)) and hi = fl(t * (1 + 2^-40)), and the guards are only
// armed when thr and e are finite NORMAL positive numbers and 2^-1000 <= t < inf (so no product above over- or underflows; otherwise lo = 0 and
// hi = +inf, which no |num| is below or above, and every point takes the exact division):
//   t <= thr*e*(1 + u) and lo <= t*(1 - 2^-40)*(1 + u), so num < lo gives num / e < thr*(1 - 2^-40)*(1 + u)^2 < thr*(1 - 2^-41).  The largest
//   double below thr is >= thr*(1 - 2^-52) > thr*(1 - 2^-41); rounding is monotone, so q <= that double < thr: an inlier.
//   Likewise num > hi gives num / e > thr*(1 + 2^-40)*(1 - u)^2 > thr*(1 + 2^-41) > the smallest double above thr (<= thr*(1 + 2^-52)), so
//   q > thr (or q overflows to +inf): not an inlier.  NaN compares false both ways and lands on the exact path, where NaN < thr is false.
//   Between lo and hi the IEEE division itself decides (on uniform data: none of 1.3*10^7 pairs).
// The line compares s = (cr.x^2 + cr.y^2) + cr.z^2 -- the very value the reference takes the root of -- with lo2 = fl(fl(t*t) * (1 - 2^-38)) and
// hi2 = fl(fl(t*t) * (1 + 2^-38)), t = fl(thr * len): lo2 <= (thr*len)^2 * (1 - 2^-38) * (1 + u)^4, so s < lo2 gives sqrt(s) < thr*len*(1 - 2^-39 + 2^-51),
// fl(sqrt(s)) <= that * (1 + u), and the quotient by len stays below thr*(1 - 2^-40) < pred(thr); symmetric above.  Same arming rule, on t and t*t.
#include "device_sort.hpp"
#include "positions_device.hpp"

#include <algorithm>

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kPointsPerLane = pstk::kRansacPointsPerWave / 64;
constexpr double kMinNormal = 2.2250738585072014e-308;

struct PlaneRec { double a, b, c, d, e, lo, hi, thr; };                                  // 64 bytes
struct LineRec { double f[3], s[3], dv[3], len, lo2, hi2, thr, pad[3]; };                // 128 bytes
// a record through the constant address space (wave-uniform index: scalar loads)
template <typename Rec>
__device__ __forceinline__ Rec load_rec_uniform(const Rec* table, uint32_t h) {
  const PST_AS_CONST double* q = (const PST_AS_CONST double*)(table + h);
  Rec r;
  double* d = reinterpret_cast<double*>(&r);
#pragma unroll
  for (uint32_t i = 0; i < sizeof(Rec) / sizeof(double); ++i) d[i] = q[i];
  return r;
}

__device__ __forceinline__ bool normal_positive(double v) { return v >= kMinNormal && v < kInf; }

__device__ __forceinline__ PlaneRec make_plane_rec(double a, double b, double c, double d, double thr) {
  PlaneRec r;
  r.a = a; r.b = b; r.c = c; r.d = d; r.thr = thr;
  r.e = __builtin_sqrt((a * a + b * b) + c * c);
  const double t = thr * r.e;
  const bool armed = normal_positive(thr) && normal_positive(r.e) && t >= 0x1p-1000 && t < kInf;
  r.lo = armed ? t * (1.0 - 0x1p-40) : 0.0;
  r.hi = armed ? t * (1.0 + 0x1p-40) : kInf;
  return r;
}
__device__ __forceinline__ LineRec make_line_rec(const double f[3], const double s[3], double thr) {
  LineRec r;
  for (int c = 0; c < 3; ++c) { r.f[c] = f[c]; r.s[c] = s[c]; r.dv[c] = s[c] - f[c]; r.pad[c] = 0.0; }
  r.thr = thr;
  r.len = __builtin_sqrt((r.dv[0] * r.dv[0] + r.dv[1] * r.dv[1]) + r.dv[2] * r.dv[2]);
  const double t = thr * r.len, t2 = t * t;
  const bool armed = normal_positive(thr) && normal_positive(r.len) && t >= 0x1p-500 && t < kInf && t2 >= 0x1p-1000 && t2 < kInf;
  r.lo2 = armed ? t2 * (1.0 - 0x1p-38) : 0.0;
  r.hi2 = armed ? t2 * (1.0 + 0x1p-38) : kInf;
  return r;
}

// ---- the predicate: ONE set of device functions for the scoring, mask and index kernels -------------------------------------------------
// value(): the quantity the guards look at; exact(): the reference's comparison on that value; inlier() = guards, then exact().
struct PlaneModel {
  typedef PlaneRec Rec;
  static __device__ __forceinline__ double value(const Rec& r, double x, double y, double z) {
    return __builtin_fabs(((r.a * x + r.b * y) + r.c * z) + r.d);
  }
  static __device__ __forceinline__ double lo(const Rec& r) { return r.lo; }
  static __device__ __forceinline__ double hi(const Rec& r) { return r.hi; }
  static __device__ __forceinline__ bool exact(const Rec& r, double num) { return num / r.e < r.thr; }
};
struct LineModel {
  typedef LineRec Rec;
  static __device__ __forceinline__ double value(const Rec& r, double x, double y, double z) {
    const double wx = r.f[0] - x, wy = r.f[1] - y, wz = r.f[2] - z;
    const double cx = r.dv[1] * wz - r.dv[2] * wy, cy = r.dv[2] * wx - r.dv[0] * wz, cz = r.dv[0] * wy - r.dv[1] * wx;
    return (cx * cx + cy * cy) + cz * cz;
  }
  static __device__ __forceinline__ double lo(const Rec& r) { return r.lo2; }
  static __device__ __forceinline__ double hi(const Rec& r) { return r.hi2; }
  static __device__ __forceinline__ bool exact(const Rec& r, double s) { return __builtin_sqrt(s) / r.len < r.thr; }
};
template <typename M>
__device__ __forceinline__ bool inlier(const typename M::Rec& r, double x, double y, double z) {
  const double v = M::value(r, x, y, z);
  if (v < M::lo(r)) return true;
  if (v > M::hi(r)) return false;
  return M::exact(r, v);
}

// ---- hypothesis table -----------------------------------------------------------------------------------------------------------------------
// one lane per hypothesis: gathers the sampled positions, writes the record and zeroes the hypothesis' ranking
__global__ __launch_bounds__(kBlock) void ransac_plane_table_kernel(Pos pos, const uint64_t* __restrict__ samples, uint32_t nh, double thr,
                                                                    PlaneRec* __restrict__ recs, unsigned long long* __restrict__ rank) {
  const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= nh) return;
  double p1[3], p2[3], p3[3];
  load_point(pos, samples[3 * (uint64_t)h], p1[0], p1[1], p1[2]);
  load_point(pos, samples[3 * (uint64_t)h + 1], p2[0], p2[1], p2[2]);
  load_point(pos, samples[3 * (uint64_t)h + 2], p3[0], p3[1], p3[2]);
  const double ux = p2[0] - p1[0], uy = p2[1] - p1[1], uz = p2[2] - p1[2];
  const double vx = p3[0] - p1[0], vy = p3[1] - p1[1], vz = p3[2] - p1[2];
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double d = -((nx * p1[0] + ny * p1[1]) + nz * p1[2]);
  recs[h] = make_plane_rec(nx, ny, nz, d, thr);
  rank[h] = 0;
}
__global__ __launch_bounds__(kBlock) void ransac_line_table_kernel(Pos pos, const uint64_t* __restrict__ samples, uint32_t nh, double thr,
                                                                   LineRec* __restrict__ recs, unsigned long long* __restrict__ rank) {
  const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= nh) return;
  double f[3], s[3];
  load_point(pos, samples[2 * (uint64_t)h], f[0], f[1], f[2]);
  load_point(pos, samples[2 * (uint64_t)h + 1], s[0], s[1], s[2]);
  recs[h] = make_line_rec(f, s, thr);
  rank[h] = 0;
}
// the record of a caller's model (mask / index entry points): the same make_*_rec on the device, so the guards and e are the scoring kernel's
struct Model6 { double v[6]; };
__global__ void ransac_plane_model_kernel(Model6 m, double thr, PlaneRec* __restrict__ rec) { *rec = make_plane_rec(m.v[0], m.v[1], m.v[2], m.v[3], thr); }
__global__ void ransac_line_model_kernel(Model6 m, double thr, LineRec* __restrict__ rec) { *rec = make_line_rec(m.v, m.v + 3, thr); }

// ---- scoring: the hot path ------------------------------------------------------------------------------------------------------------------
// One wave per tile of kRansacPointsPerWave points, kPointsPerLane of them per lane in registers (12 VGPR pairs).  The wave then walks the
// whole batch of hypotheses; a record is wave-uniform and comes in through scalar loads from the constant address space (the table is
// written by an earlier launch and only read here).  Per point and hypothesis the plane costs 6 f64 VALU instructions + 2 compares (the
// line 17 + 2); inliers are counted with ballot + popcount on the scalar unit.  The count of hypothesis h0 + j is folded into lane j's
// register (one select + add per hypothesis and tile) and once per 64 hypotheses and tile into the wave's own LDS counters, so the positions
// are read from HBM once per batch of up to kRansacBatch hypotheses.  At the end the block adds its four waves' counters and issues at most
// one 64-bit atomic per hypothesis.
template <typename M>
__global__ __launch_bounds__(kBlock) void ransac_score_kernel(Pos pos, uint64_t n, const typename M::Rec* __restrict__ recs, uint32_t nh,
                                                              unsigned long long* __restrict__ rank) {
  __shared__ uint32_t counts[kBlock / 64][pstk::kRansacBatch];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t nh64 = (nh + 63u) & ~63u;
  for (uint32_t h = lane; h < nh64; h += 64) counts[wave][h] = 0;
  const uint64_t n_tiles = (n + pstk::kRansacPointsPerWave - 1) / pstk::kRansacPointsPerWave;
  const double nan = __builtin_nan("");
  const uint64_t all = __ballot(true);  // the whole wave runs every iteration of the loops below
  for (uint64_t tile = (uint64_t)blockIdx.x * (kBlock / 64) + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * (kBlock / 64)) {
    double x[kPointsPerLane], y[kPointsPerLane], z[kPointsPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kPointsPerLane; ++k) {
      const uint64_t i = tile * pstk::kRansacPointsPerWave + k * 64 + lane;
      x[k] = y[k] = z[k] = nan;  // past the end: a NaN is an inlier of nothing
      if (i < n) load_point(pos, i, x[k], y[k], z[k]);
    }
    for (uint32_t h0 = 0; h0 < nh; h0 += 64) {
      const uint32_t hb = min(64u, nh - h0);
      uint32_t mine = 0;
      typename M::Rec next = load_rec_uniform(recs, h0);
      for (uint32_t j = 0; j < hb; ++j) {
        const typename M::Rec r = next;
        next = load_rec_uniform(recs, h0 + min(j + 1, hb - 1));  // the next record's scalar loads fly during this one's arithmetic
        double v[kPointsPerLane];
        uint64_t open[kPointsPerLane], any_open = 0;
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPointsPerLane; ++k) {
          v[k] = M::value(r, x[k], y[k], z[k]);
          const uint64_t in = __ballot(v[k] < M::lo(r)), out = __ballot(v[k] > M::hi(r));  // two compares; a NaN sets neither bit
          c += (uint32_t)__popcll(in);
          open[k] = ~(in | out) & all;
          any_open |= open[k];
        }
        if (any_open != 0) {  // wave-uniform: the division (and the line's root) stay out of the loop's straight path
#pragma unroll
          for (uint32_t k = 0; k < kPointsPerLane; ++k) {
            const bool undecided = (open[k] >> lane) & 1u;
            c += (uint32_t)__popcll(__ballot(undecided && M::exact(r, v[k])));
          }
        }
        mine += lane == j ? c : 0u;
      }
      counts[wave][h0 + lane] += mine;
    }
  }
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < nh; h += kBlock) {
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) s += counts[w][h];
    if (s) atomicAdd(&rank[h], s);
  }
}

// ---- arg-max: highest ranking, the LAST such iteration on ties (Iterator::max_by) -------------------------------------------------------------
// out: {best iteration, its ranking} as two u64, then the model (plane: a b c d; line: first, second) as doubles
template <typename Rec, bool LINE>
__global__ __launch_bounds__(kBlock) void ransac_argmax_kernel(const unsigned long long* __restrict__ rank, const Rec* __restrict__ recs, uint64_t nh,
                                                               unsigned long long* __restrict__ out) {
  __shared__ unsigned long long best_r[kBlock], best_i[kBlock];
  unsigned long long br = 0, bi = 0;
  bool any = false;
  for (uint64_t h = threadIdx.x; h < nh; h += kBlock) {  // ascending h per thread: >= keeps the later one
    const unsigned long long r = rank[h];
    if (!any || r >= br) { br = r; bi = h; any = true; }
  }
  best_r[threadIdx.x] = br;
  best_i[threadIdx.x] = any ? bi : ~0ull;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t t = 0; t < kBlock; ++t) {
      if (best_i[t] == ~0ull) continue;
      if (!any || best_r[t] > br || (best_r[t] == br && best_i[t] > bi)) { br = best_r[t]; bi = best_i[t]; any = true; }
    }
    out[0] = bi;
    out[1] = br;
    double* m = (double*)(out + 2);
    if constexpr (LINE) {
      for (int c = 0; c < 3; ++c) { m[c] = recs[bi].f[c]; m[3 + c] = recs[bi].s[c]; }
    } else {
      m[0] = recs[bi].a; m[1] = recs[bi].b; m[2] = recs[bi].c; m[3] = recs[bi].d;
    }
  }
}

// ---- inlier passes --------------------------------------------------------------------------------------------------------------------------
template <typename M>
__global__ __launch_bounds__(kBlock) void ransac_mask_kernel(Pos pos, uint64_t n, const typename M::Rec* __restrict__ rec, uint8_t* __restrict__ mask) {
  const typename M::Rec r = *rec;
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    double x, y, z;
    load_point(pos, i, x, y, z);
    mask[i] = inlier<M>(r, x, y, z) ? 1 : 0;
  }
}

// ordered compaction of 0..n under the predicate: a block owns kRansacPointsPerBlock consecutive points, a thread four consecutive ones.
// WRITE = false: counts[block] = inliers of the block.  WRITE = true: offsets[] is the exclusive scan of those counts (radix_sort.hip).
template <typename M, bool WRITE>
__global__ __launch_bounds__(kBlock) void ransac_index_kernel(Pos pos, uint64_t n, const typename M::Rec* __restrict__ rec, uint32_t* __restrict__ counts,
                                                              const unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ indices) {
  constexpr uint32_t kPer = pstk::kRansacPointsPerBlock / kBlock;
  __shared__ uint32_t wave_sum[kBlock / 64];
  const typename M::Rec r = *rec;
  const uint64_t first = (uint64_t)blockIdx.x * pstk::kRansacPointsPerBlock + (uint64_t)threadIdx.x * kPer;
  bool in[kPer];
  uint32_t c = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    in[k] = false;
    if (first + k < n) {
      double x, y, z;
      load_point(pos, first + k, x, y, z);
      in[k] = inlier<M>(r, x, y, z);
    }
    c += in[k] ? 1u : 0u;
  }
  // inclusive scan of c over the wave, then over the block's four waves
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
    if ((int)lane >= off) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kBlock / 64; ++w) {
    before += w < wave ? wave_sum[w] : 0u;
    total += wave_sum[w];
  }
  if constexpr (!WRITE) {
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
  } else {
    unsigned long long at = offsets[blockIdx.x] + before + (incl - c);
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (in[k]) indices[at++] = first + k;
  }
}

template <typename M>
bool run_model_rec(const double* model, double thr, typename M::Rec* rec, hipStream_t s) {
  Model6 m{};
  const int nm = std::is_same<M, PlaneModel>::value ? 4 : 6;
  for (int c = 0; c < nm; ++c) m.v[c] = model[c];
  if constexpr (std::is_same<M, PlaneModel>::value) hipLaunchKernelGGL(ransac_plane_model_kernel, dim3(1), dim3(1), 0, s, m, thr, rec);
  else hipLaunchKernelGGL(ransac_line_model_kernel, dim3(1), dim3(1), 0, s, m, thr, rec);
  return launched();
}

template <typename M, bool LINE>
bool fit(const Pos& pos, uint64_t n, double thr, const uint64_t* samples_dev, uint64_t iterations, void* recs_v, unsigned long long* rank,
         unsigned long long* out, hipStream_t s) {
  typedef typename M::Rec Rec;
  Rec* recs = (Rec*)recs_v;
  const unsigned tgrid = (unsigned)((iterations + kBlock - 1) / kBlock);
  if constexpr (LINE) hipLaunchKernelGGL(ransac_line_table_kernel, dim3(tgrid), dim3(kBlock), 0, s, pos, samples_dev, (uint32_t)iterations, thr, recs, rank);
  else hipLaunchKernelGGL(ransac_plane_table_kernel, dim3(tgrid), dim3(kBlock), 0, s, pos, samples_dev, (uint32_t)iterations, thr, recs, rank);
  if (!launched()) return false;
  const uint64_t blocks_needed = (n + pstk::kRansacPointsPerBlock - 1) / pstk::kRansacPointsPerBlock;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks_needed, (uint64_t)pstk::device_cus() * pstk::kRansacBlocksPerCu));
  for (uint64_t h0 = 0; h0 < iterations; h0 += pstk::kRansacBatch) {
    const uint32_t nh = (uint32_t)std::min<uint64_t>(pstk::kRansacBatch, iterations - h0);
    hipLaunchKernelGGL(ransac_score_kernel<M>, dim3(grid), dim3(kBlock), 0, s, pos, n, (const Rec*)(recs + h0), nh, rank + h0);
    if (!launched()) return false;
  }
  hipLaunchKernelGGL((ransac_argmax_kernel<Rec, LINE>), dim3(1), dim3(kBlock), 0, s, rank, recs, iterations, out);
  return launched();
}

template <typename M>
bool mask(const Pos& pos, uint64_t n, const double* model, double thr, void* rec_scratch, uint8_t* mask_dev, hipStream_t s) {
  typedef typename M::Rec Rec;
  if (!run_model_rec<M>(model, thr, (Rec*)rec_scratch, s)) return false;
  if (n == 0) return true;
  const unsigned grid = (unsigned)std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)pstk::device_cus() * 16);
  hipLaunchKernelGGL(ransac_mask_kernel<M>, dim3(grid), dim3(kBlock), 0, s, pos, n, (const Rec*)rec_scratch, mask_dev);
  return launched();
}

template <typename M>
bool index_pass(const Pos& pos, uint64_t n, const void* rec, uint32_t* counts, const unsigned long long* offsets, unsigned long long* indices, bool write,
                hipStream_t s) {
  typedef typename M::Rec Rec;
  const unsigned grid = (unsigned)((n + pstk::kRansacPointsPerBlock - 1) / pstk::kRansacPointsPerBlock);
  if (write) hipLaunchKernelGGL((ransac_index_kernel<M, true>), dim3(grid), dim3(kBlock), 0, s, pos, n, (const Rec*)rec, counts, offsets, indices);
  else hipLaunchKernelGGL((ransac_index_kernel<M, false>), dim3(grid), dim3(kBlock), 0, s, pos, n, (const Rec*)rec, counts, offsets, indices);
  return launched();
}

}  // namespace

namespace pstk {

size_t ransac_record_bytes(bool line) { return line ? sizeof(LineRec) : sizeof(PlaneRec); }

bool ransac_fit(bool line, const Positions& p, double thr, const uint64_t* samples_dev, uint64_t iterations, void* recs, unsigned long long* rank,
                unsigned long long* out8, hipStream_t stream) {
  return line ? fit<LineModel, true>(pos_of(p), p.n, thr, samples_dev, iterations, recs, rank, out8, stream)
              : fit<PlaneModel, false>(pos_of(p), p.n, thr, samples_dev, iterations, recs, rank, out8, stream);
}

bool ransac_mask(bool line, const Positions& p, const double* model, double thr, void* rec_scratch, uint8_t* mask_dev, hipStream_t stream) {
  return line ? mask<LineModel>(pos_of(p), p.n, model, thr, rec_scratch, mask_dev, stream) : mask<PlaneModel>(pos_of(p), p.n, model, thr, rec_scratch, mask_dev, stream);
}

bool ransac_model_record(bool line, const double* model, double thr, void* rec_scratch, hipStream_t stream) {
  return line ? run_model_rec<LineModel>(model, thr, (LineRec*)rec_scratch, stream) : run_model_rec<PlaneModel>(model, thr, (PlaneRec*)rec_scratch, stream);
}

bool ransac_index_pass(bool line, const Positions& p, const void* rec, uint32_t* counts, const unsigned long long* offsets, unsigned long long* indices, bool write,
                       hipStream_t stream) {
  return line ? index_pass<LineModel>(pos_of(p), p.n, rec, counts, offsets, indices, write, stream)
              : index_pass<PlaneModel>(pos_of(p), p.n, rec, counts, offsets, indices, write, stream);
}

}  // namespace pstk
