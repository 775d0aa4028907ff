// Point-in-polygon ids and masks: polygon crop and overlay (include/pasture_amd.h, "Polygon crop and overlay"; the index is built on the host,
// polygon_index.hpp; the checks and the set's device memory are in crop_api.cpp).
//
// The definition, which both bodies below and tests/crop_ref.py evaluate to the same bits.  An entry is a canonical edge {lo, hi}, lo.y < hi.y.
// A point p with finite x and y CROSSES it iff lo.y <= p.y, p.y < hi.y and d > 0, d finite, where
//   d = (hi.x - lo.x) * (p.y - lo.y) - (p.x - lo.x) * (hi.y - lo.y)
// in f64 with one rounding per operation (this file is compiled without contraction): four subtractions, two products, one subtraction.  p is
// in a polygon iff it crosses an odd number of its entries; its id is the smallest such polygon.  z is never read.
//
// One launch per query, one of two bodies:
//   flat    a workgroup copies ALL entries (at most kCropFlatMaxEdges, 36 bytes each) into LDS once and serves kCropFlatPointsPerBlock points,
//           four per lane in registers.  The loop over the entries is the same for every lane: each LDS read is one address for the whole
//           wave (a broadcast), the polygon index is made a scalar, and the parity of the current polygon is committed where that index
//           changes -- a uniform branch.  A lane whose point has its polygon only stops updating the id.
//   banded  one lane per point.  A point outside the box in y, or at or beyond it on the right, crosses nothing (below); any other point walks
//           the list of its y-band (polygon_index.hpp: band_of is monotone, so the list holds every entry the point can cross) and stops at the
//           first polygon boundary where the parity is odd.  The lists are read as 32-byte aligned records and a u32 array beside them.
// Per point and entry: 7 f64 operations and 3 compares (about ten operations); traffic: the 24-byte position lines in, 1 or 4 bytes out.
//
// The box tests of the banded body change no result:
//   p.y < ymin   no entry has lo.y <= p.y;  p.y >= ymax   no entry has p.y < hi.y.
//   p.x >= xmax  with lo.y <= p.y < hi.y: A = fl(hi.x - lo.x) <= u = fl(p.x - lo.x) and 0 <= t = fl(p.y - lo.y) <= h = fl(hi.y - lo.y), 0 < h,
//                because a rounded subtraction is monotone in either operand and p.x >= hi.x, p.x >= lo.x, p.y < hi.y.  For A <= 0 the first
//                product is <= 0 <= the second; for A > 0, A * t <= u * h in the reals and rounding keeps the order.  So the rounded products
//                are ordered, fl(A * t) <= fl(u * h), and d is <= 0 -- or a NaN when both overflowed, which is not a crossing either.
//   There is NO test on p.x < xmin: for such a point d > 0 holds in the reals, but the two products may round to the same value (or underflow
//   together) and give d == 0, which the definition answers with "no crossing".
#include "polygon_index.hpp"
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kNo = pstk::kCropNoPolygon;
constexpr uint32_t kFlatPpb = pstk::kCropFlatPointsPerBlock, kFlatPerLane = kFlatPpb / kBlock;
constexpr uint32_t kBandedPpb = pstk::kCropBandedPointsPerBlock;
static_assert(kBandedPpb == (uint32_t)kBlock && kFlatPpb % kBlock == 0, "one lane per point / whole points per lane");
static_assert(pstk::kCropFlatMaxEdges * 36 <= 64 * 1024, "the flat body's LDS copy is dynamic LDS without a per-kernel attribute");

using Set = pstk::CropSet;

__device__ __forceinline__ bool crosses(double lox, double loy, double hix, double hiy, double x, double y) {
  const double a = hix - lox, t = y - loy, u = x - lox, h = hiy - loy;
  const double p1 = a * t, p2 = u * h;
  const double d = p1 - p2;
  return loy <= y && y < hiy && d > 0.0 && d <= kF64Max;
}

// the selected points of a wave (every lane calls it), for the wave's one integer atomic
__device__ __forceinline__ uint32_t selected_in_wave(bool selected) { return (uint32_t)__popcll(__ballot(selected)); }

__device__ __forceinline__ void write_result(uint64_t i, uint32_t id, uint32_t* __restrict__ ids, uint8_t* __restrict__ mask, uint32_t outside, bool& selected) {
  const bool inside = id != kNo;
  if (ids) ids[i] = id;
  selected = inside;
  if (mask) {
    selected = inside != (outside != 0);
    mask[i] = selected ? 1 : 0;
  }
}

__global__ __launch_bounds__(kBlock) void crop_flat_kernel(Pos pos, uint64_t n, Set set, uint32_t* __restrict__ ids, uint8_t* __restrict__ mask, uint32_t outside,
                                                           unsigned long long* count) {
  extern __shared__ __attribute__((aligned(16))) double lds_records[];  // 4 * E doubles, then E polygon indices
  const uint32_t n_entries = set.n_records;
  uint32_t* lds_polygon = (uint32_t*)(lds_records + 4 * (size_t)n_entries);
  for (uint32_t k = threadIdx.x; k < 4 * n_entries; k += kBlock) lds_records[k] = set.records[k];
  for (uint32_t k = threadIdx.x; k < n_entries; k += kBlock) lds_polygon[k] = set.polygon[k];
  __syncthreads();

  const uint64_t first = (uint64_t)blockIdx.x * kFlatPpb;
  double x[kFlatPerLane], y[kFlatPerLane];
  uint32_t id[kFlatPerLane];
  bool odd[kFlatPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kFlatPerLane; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    x[j] = y[j] = kInf;  // (a point that is not finite crosses nothing: every comparison with its y fails)
    if (i < n) {
      cgptr_t q = pos.base + i * pos.stride;
      const double px = load_un<double>(q), py = load_un<double>(q + 8);
      if (finite(px) && finite(py)) { x[j] = px; y[j] = py; }
    }
    id[j] = kNo;
    odd[j] = false;
  }
  uint32_t cur = kNo;
  for (uint32_t e = 0; e < n_entries; ++e) {
    const uint32_t p = __builtin_amdgcn_readfirstlane(lds_polygon[e]);
    if (p != cur) {  // a polygon boundary: the same for every lane
#pragma unroll
      for (uint32_t j = 0; j < kFlatPerLane; ++j) {
        id[j] = (id[j] == kNo && odd[j]) ? cur : id[j];
        odd[j] = false;
      }
      cur = p;
    }
    const double lox = lds_records[4 * e], loy = lds_records[4 * e + 1], hix = lds_records[4 * e + 2], hiy = lds_records[4 * e + 3];
#pragma unroll
    for (uint32_t j = 0; j < kFlatPerLane; ++j) odd[j] = odd[j] != crosses(lox, loy, hix, hiy, x[j], y[j]);
  }
  uint32_t wave_total = 0;
#pragma unroll
  for (uint32_t j = 0; j < kFlatPerLane; ++j) {
    id[j] = (id[j] == kNo && odd[j]) ? cur : id[j];
    const uint64_t i = first + j * kBlock + threadIdx.x;
    bool selected = false;
    if (i < n) write_result(i, id[j], ids, mask, outside, selected);
    wave_total += selected_in_wave(selected);
  }
  if (count && wave_total && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)wave_total);
}

__global__ __launch_bounds__(kBlock) void crop_banded_kernel(Pos pos, uint64_t n, Set set, uint32_t* __restrict__ ids, uint8_t* __restrict__ mask, uint32_t outside,
                                                             unsigned long long* count) {
  const uint64_t i = (uint64_t)blockIdx.x * kBandedPpb + threadIdx.x;
  bool selected = false;
  if (i < n) {
    cgptr_t q = pos.base + i * pos.stride;
    const double x = load_un<double>(q), y = load_un<double>(q + 8);
    uint32_t id = kNo;
    if (finite(x) && finite(y) && !(y < set.ymin) && !(y >= set.ymax) && !(x >= set.xmax)) {
      const uint32_t b = pst::polygon::band_of(pst::polygon::Bands{set.ymin, set.scale, set.bands}, y);  // < set.bands: offsets has bands + 1 entries
      const uint32_t end = set.offsets[b + 1];
      uint32_t cur = kNo;
      bool odd = false;
      for (uint32_t k = set.offsets[b]; k < end; ++k) {
        const uint32_t p = set.polygon[k];
        if (p != cur) {
          if (odd) break;  // the polygons before this one did not contain the point, `cur` does: the smallest index
          cur = p;
        }
        const double2* r = (const double2*)(set.records + 4 * (size_t)k);  // a 32-byte aligned record: two 16-byte loads
        const double2 lo = r[0], hi = r[1];
        odd = odd != crosses(lo.x, lo.y, hi.x, hi.y, x, y);
      }
      id = odd ? cur : kNo;
    }
    write_result(i, id, ids, mask, outside, selected);
  }
  const uint32_t wave_total = selected_in_wave(selected);
  if (count && wave_total && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned long long)wave_total);
}

__global__ __launch_bounds__(kBlock) void set_u8_from_ids_kernel(gptr_t base, uint64_t stride, uint64_t n, const uint32_t* __restrict__ ids,
                                                                 const uint8_t* __restrict__ values, uint32_t n_values, unsigned long long* written) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool hit = false;
  if (i < n) {
    const uint32_t id = ids[i];
    hit = id < n_values;
    if (hit) *(base + i * stride) = values[id];
  }
  const uint32_t wave_total = (uint32_t)__popcll(__ballot(hit));
  if (written && wave_total && (threadIdx.x & 63) == 0) atomicAdd(written, (unsigned long long)wave_total);
}

}  // namespace

namespace pstk {

bool crop_query(const Positions& pos, const CropSet& set, bool flat, uint32_t* ids, uint8_t* mask, int outside, unsigned long long* count, hipStream_t stream) {
  if (pos.n == 0) return true;
  if (flat) {
    if (set.n_records > kCropFlatMaxEdges) return false;  // (the LDS copy is sized by it)
    const uint32_t lds_bytes = set.n_records * 36u;
    hipLaunchKernelGGL(crop_flat_kernel, dim3(blocks_of(pos.n, kFlatPpb)), dim3(kBlock), lds_bytes, stream, pos_of(pos), pos.n, set, ids, mask, outside ? 1u : 0u, count);
  } else {
    if (set.bands == 0 || !set.offsets) return false;
    hipLaunchKernelGGL(crop_banded_kernel, dim3(blocks_of(pos.n, kBandedPpb)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, set, ids, mask, outside ? 1u : 0u, count);
  }
  return launched();
}

bool set_u8_from_ids(uint64_t addr, uint64_t stride, uint64_t n, const uint32_t* ids, const uint8_t* values, uint32_t n_values, unsigned long long* written,
                     hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(set_u8_from_ids_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, (gptr_t)addr, stride, n, ids, values, n_values, written);
  return launched();
}

}  // namespace pstk
