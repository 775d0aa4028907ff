// Gather by index -- dst[dst_first + j] = src[idx[j]] for every attribute, byte for byte -- and the key kernels of the device sort orders
// (by attribute, Morton, shuffle), for gfx950.  include/pasture_amd.h, "Gather by index and sort orders", has the definitions.
//
//   gather_kernel<SRC_AOS, DST_AOS>   a workgroup owns kReorderPointsPerBlock consecutive OUTPUT points.  Lane j reads index j once (coalesced),
//                                     an index >= src_len becomes the invalid marker: its target point is never written, the block adds its
//                                     number of such entries to the status word with one atomic.
//     columnar -> columnar            per attribute, granule k of the tile's contiguous output span is element idx[k / cnt], component k % cnt;
//                                     1- and 2-byte granules leave as whole dwords where all their points are valid.
//     columnar -> interleaved         the same loads, stored into an LDS record tile; the tile leaves with 16-byte stores (tile_store).
//     interleaved -> interleaved      lanes are assigned to (record, 16-byte piece): consecutive lanes read consecutive bytes of ONE record, so a
//                                     record's cache lines are fetched once; whole records (padding included) go through the LDS record tile.
//     interleaved -> columnar         records staged the same way, then the attributes are read out of LDS column by column.
//                                     A tile that is not wholly overwritten (padding the attributes do not cover, skipped points) is first
//                                     loaded from the target, so the bytes that are not the gather's stay what they were.
//   gather_bytes_kernel               records that do not fit the LDS tile (ByteArray attributes of several KB): a wave per output point,
//                                     attribute by attribute, dwords then bytes.  Any point size.
//   index_check_kernel                max index and number of entries >= src_len in one pass (the synchronous entry points refuse a bad list
//                                     before anything is written).
//   attribute / Morton / shuffle key kernels, invert.
// Element-granular gathers are bound by the cache lines they touch, not by the bytes they want: no MFMA, no scratch.
#include "positions_device.hpp"
#include "tile_io.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kReorderPointsPerBlock;
static_assert(kP == kBlock, "one index per lane");
constexpr unsigned long long kInvalid = ~0ull;

using pstk::GatherArgs;
using pstk::GatherAttr;

// the tile's indices into LDS, out-of-range entries as kInvalid; returns their number (block-uniform)
__device__ __forceinline__ uint32_t load_indices(const GatherArgs& a, uint64_t out0, uint32_t m, unsigned long long* s_idx, uint32_t* s_bad) {
  if (threadIdx.x == 0) *s_bad = 0;
  __syncthreads();
  unsigned long long v = kInvalid;
  if (threadIdx.x < m) {
    v = a.idx64 ? ((const unsigned long long*)a.idx)[out0 + threadIdx.x] : (unsigned long long)((const uint32_t*)a.idx)[out0 + threadIdx.x];
    if (v >= a.src_len) v = kInvalid;
  }
  s_idx[threadIdx.x] = v;
  const unsigned long long bad = __ballot(threadIdx.x < m && v == kInvalid);
  if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(s_bad, (uint32_t)__popcll(bad));
  __syncthreads();
  const uint32_t nbad = *s_bad;
  if (threadIdx.x == 0 && nbad && a.count_skipped && a.skipped) atomicAdd(a.skipped, (unsigned long long)nbad);
  return nbad;
}

__device__ __forceinline__ void split_granule(uint32_t k, uint32_t cnt, uint32_t& j, uint32_t& c) {
  if (cnt == 1) { j = k; c = 0; }
  else if (cnt == 3) { j = (k * 43691u) >> 17; c = k - 3u * j; }  // (exact below 98304: k < 3 * kP)
  else { j = k / cnt; c = k - j * cnt; }
}

template <typename U> struct LdsValue {
  static __device__ __forceinline__ U load(clptr_t p) { return lds_load<U>(p); }
  static __device__ __forceinline__ void store(lptr_t p, U v) { lds_store<U>(p, v); }
};
template <> struct LdsValue<u32x4> {
  static __device__ __forceinline__ u32x4 load(clptr_t p) {
    const uint64_t lo = lds_load<uint64_t>(p), hi = lds_load<uint64_t>(p + 8);
    return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
  }
  static __device__ __forceinline__ void store(lptr_t p, u32x4 v) {
    lds_store<uint64_t>(p, (uint64_t)v.x | ((uint64_t)v.y << 32));
    lds_store<uint64_t>(p + 8, (uint64_t)v.z | ((uint64_t)v.w << 32));
  }
};

// The m * cnt granules of one attribute of m consecutive output points, to the column span at dst.  fetch(j, c): component c of the source
// point the tile's j-th index names; it is called for valid j only.
template <typename U, typename F>
__device__ __forceinline__ void store_column(gptr_t dst, uint32_t cnt, uint32_t m, const unsigned long long* sidx, F&& fetch) {
  const uint32_t total = m * cnt;
  constexpr uint32_t PACK = sizeof(U) >= 4 ? 1u : 4u / (uint32_t)sizeof(U);
  if constexpr (PACK > 1) {
    auto one = [&](uint32_t k) {
      uint32_t j, c;
      split_granule(k, cnt, j, c);
      if (sidx[j] != kInvalid) store_un<U>(dst + k * (uint32_t)sizeof(U), fetch(j, c));
    };
    const uint32_t head = ((0u - (uint32_t)(uintptr_t)dst) & 3u) / (uint32_t)sizeof(U);  // granules before the first aligned dword
    const uint32_t h = head < total ? head : total;
    if (threadIdx.x < h) one(threadIdx.x);
    const uint32_t nd = (total - h) / PACK;
    for (uint32_t q = threadIdx.x; q < nd; q += kBlock) {
      const uint32_t k0 = h + q * PACK;
      uint32_t packed = 0;
      bool all = true;
#pragma unroll
      for (uint32_t i = 0; i < PACK; ++i) {
        uint32_t j, c;
        split_granule(k0 + i, cnt, j, c);
        if (sidx[j] != kInvalid) packed |= (uint32_t)fetch(j, c) << (8u * (uint32_t)sizeof(U) * i);
        else all = false;
      }
      if (all) store_un<uint32_t>(dst + k0 * (uint32_t)sizeof(U), packed);
      else {
#pragma unroll
        for (uint32_t i = 0; i < PACK; ++i) {
          uint32_t j, c;
          split_granule(k0 + i, cnt, j, c);
          if (sidx[j] != kInvalid) store_un<U>(dst + (k0 + i) * (uint32_t)sizeof(U), (U)(packed >> (8u * (uint32_t)sizeof(U) * i)));
        }
      }
    }
    for (uint32_t k = h + nd * PACK + threadIdx.x; k < total; k += kBlock) one(k);
  } else {
    constexpr uint32_t kBatch = 4;  // loads in flight per lane before the first store
    for (uint32_t k0 = threadIdx.x; k0 < total; k0 += kBatch * kBlock) {
      U v[kBatch];
      bool ok[kBatch];
#pragma unroll
      for (uint32_t u = 0; u < kBatch; ++u) {
        const uint32_t k = k0 + u * kBlock;
        ok[u] = false;
        if (k < total) {
          uint32_t j, c;
          split_granule(k, cnt, j, c);
          if (sidx[j] != kInvalid) { v[u] = fetch(j, c); ok[u] = true; }
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kBatch; ++u)
        if (ok[u]) store_un<U>(dst + (uint64_t)(k0 + u * kBlock) * sizeof(U), v[u]);
    }
  }
}

// the same granules into the LDS record tile: record j of the pass at rec0 + j * stride
template <typename U, typename F>
__device__ __forceinline__ void store_records(lptr_t rec0, uint32_t stride, uint32_t offset, uint32_t cnt, uint32_t m, const unsigned long long* sidx, F&& fetch) {
  const uint32_t total = m * cnt;
  constexpr uint32_t kBatch = 4;
  for (uint32_t k0 = threadIdx.x; k0 < total; k0 += kBatch * kBlock) {
    U v[kBatch];
    uint32_t at[kBatch];
    bool ok[kBatch];
#pragma unroll
    for (uint32_t u = 0; u < kBatch; ++u) {
      const uint32_t k = k0 + u * kBlock;
      ok[u] = false;
      at[u] = 0;
      if (k < total) {
        uint32_t j, c;
        split_granule(k, cnt, j, c);
        at[u] = j * stride + offset + c * (uint32_t)sizeof(U);
        if (sidx[j] != kInvalid) { v[u] = fetch(j, c); ok[u] = true; }
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kBatch; ++u)
      if (ok[u]) LdsValue<U>::store(rec0 + at[u], v[u]);
  }
}

// granule type of an attribute: the largest power of two up to 16 that divides its size
template <typename F>
__device__ __forceinline__ void dispatch_unit(uint32_t size, F&& f) {
  if ((size & 15u) == 0) f(u32x4{});
  else if ((size & 7u) == 0) f(uint64_t{});
  else if ((size & 3u) == 0) f(uint32_t{});
  else if ((size & 1u) == 0) f(uint16_t{});
  else f(uint8_t{});
}

// Whole source records of the pass into the LDS tile, lanes over (record, 16-byte piece).  The last piece of a record is read in pieces of
// 8, 4, 2 and 1 bytes: nothing beyond the record is read.
__device__ __forceinline__ void stage_records(const GatherArgs& a, lptr_t rec0, uint32_t m, const unsigned long long* sidx) {
  const uint32_t stride = a.stride, pieces = (stride + 15u) >> 4, total = m * pieces;
  for (uint32_t k = threadIdx.x; k < total; k += kBlock) {
    const uint32_t j = k / pieces, p = k - j * pieces;
    const unsigned long long i = sidx[j];
    if (i == kInvalid) continue;
    cgptr_t s = (cgptr_t)as_global(a.src_rec + i * stride + p * 16u);
    lptr_t d = rec0 + j * stride + p * 16u;
    const uint32_t nb = stride - p * 16u;
    if (nb >= 16u) { LdsValue<u32x4>::store(d, load_un<u32x4>(s)); continue; }
    uint32_t o = 0;
    if (nb & 8u) { lds_store<uint64_t>(d, load_un<uint64_t>(s)); o = 8; }
    if (nb & 4u) { lds_store<uint32_t>(d + o, load_un<uint32_t>(s + o)); o += 4; }
    if (nb & 2u) { lds_store<uint16_t>(d + o, load_un<uint16_t>(s + o)); o += 2; }
    if (nb & 1u) d[o] = s[o];
  }
}

template <bool SRC_AOS, bool DST_AOS>
__global__ __launch_bounds__(kBlock) void gather_kernel(const GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  __shared__ unsigned long long s_idx[kP];
  __shared__ uint32_t s_bad;
  const uint64_t out0 = (uint64_t)blockIdx.x * kP;
  const uint32_t m = (uint32_t)((a.count - out0) < kP ? (a.count - out0) : kP);
  const uint32_t nbad = load_indices(a, out0, m, s_idx, &s_bad);
  if (nbad == m) return;  // (block-uniform) nothing to write

  if constexpr (!SRC_AOS && !DST_AOS) {
    for (uint32_t ai = 0; ai < a.n_attrs; ++ai) {
      const GatherAttr at = a.attrs[ai];
      cgptr_t src = (cgptr_t)as_global(at.src);
      dispatch_unit(at.size, [&](auto tag) {
        using U = decltype(tag);
        store_column<U>(as_global(at.dst) + out0 * at.dst_stride, at.size / (uint32_t)sizeof(U), m, s_idx,
                        [&](uint32_t j, uint32_t c) { return load_un<U>(src + (s_idx[j] * at.src_stride + c * (uint32_t)sizeof(U))); });
      });
    }
  } else {
    lptr_t lds = (lptr_t)lds_raw;
    const uint32_t stride = a.stride;
    for (uint32_t j0 = 0; j0 < m; j0 += a.chunk) {
      const uint32_t cm = (m - j0) < a.chunk ? (m - j0) : a.chunk;
      const unsigned long long* sidx = s_idx + j0;
      uint32_t mis = 0;
      uint64_t ga = 0;
      if constexpr (DST_AOS) {
        ga = a.dst_rec + (out0 + j0) * stride;
        mis = (uint32_t)(ga & 15u);
        // a tile that will not be overwritten whole keeps the target's bytes (a tile of whole records from an interleaved source has no
        // uncovered padding)
        if (nbad || (!SRC_AOS && !a.dst_covered)) {
          tile_load<kBlock>(lds, (cgptr_t)as_global(ga - mis), (mis + cm * stride + 15u) & ~15u);
          wait_tile_loads();
          __syncthreads();
        }
      }
      lptr_t rec0 = lds + mis;
      if constexpr (SRC_AOS) {
        stage_records(a, rec0, cm, sidx);
      } else {
        for (uint32_t ai = 0; ai < a.n_attrs; ++ai) {
          const GatherAttr at = a.attrs[ai];
          cgptr_t src = (cgptr_t)as_global(at.src);
          dispatch_unit(at.size, [&](auto tag) {
            using U = decltype(tag);
            store_records<U>(rec0, stride, at.offset, at.size / (uint32_t)sizeof(U), cm, sidx,
                             [&](uint32_t j, uint32_t c) { return load_un<U>(src + (sidx[j] * at.src_stride + c * (uint32_t)sizeof(U))); });
          });
        }
      }
      __syncthreads();
      if constexpr (DST_AOS) {
        tile_store<kBlock>((clptr_t)lds, as_global(ga - mis), mis, cm * stride);
      } else {
        for (uint32_t ai = 0; ai < a.n_attrs; ++ai) {
          const GatherAttr at = a.attrs[ai];
          dispatch_unit(at.size, [&](auto tag) {
            using U = decltype(tag);
            store_column<U>(as_global(at.dst) + (out0 + j0) * at.dst_stride, at.size / (uint32_t)sizeof(U), cm, sidx,
                            [&](uint32_t j, uint32_t c) { return LdsValue<U>::load((clptr_t)rec0 + (j * stride + at.offset + c * (uint32_t)sizeof(U))); });
          });
        }
      }
      if (j0 + a.chunk < m) __syncthreads();  // the next pass overwrites the record tile
    }
  }
}

// any record size: wave w of the block takes the output points w, w + 4, ...; per attribute the lanes copy dwords, then the last bytes
__global__ __launch_bounds__(kBlock) void gather_bytes_kernel(const GatherArgs a) {
  __shared__ unsigned long long s_idx[kP];
  __shared__ uint32_t s_bad;
  const uint64_t out0 = (uint64_t)blockIdx.x * kP;
  const uint32_t m = (uint32_t)((a.count - out0) < kP ? (a.count - out0) : kP);
  load_indices(a, out0, m, s_idx, &s_bad);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t j = threadIdx.x >> 6; j < m; j += kBlock / 64) {
    const unsigned long long i = s_idx[j];
    if (i == kInvalid) continue;
    for (uint32_t ai = 0; ai < a.n_attrs; ++ai) {
      const GatherAttr at = a.attrs[ai];
      cgptr_t s = (cgptr_t)as_global(at.src + i * at.src_stride);
      gptr_t d = as_global(at.dst + (out0 + j) * at.dst_stride);
      const uint32_t nd = at.size >> 2;
      for (uint32_t q = lane; q < nd; q += 64u) store_un<uint32_t>(d + 4u * q, load_un<uint32_t>(s + 4u * q));
      for (uint32_t b = (nd << 2) + lane; b < at.size; b += 64u) d[b] = s[b];
    }
  }
}

__global__ __launch_bounds__(kBlock) void index_check_kernel(const void* __restrict__ idx, uint32_t idx64, uint64_t count, uint64_t src_len,
                                                             unsigned long long* __restrict__ out2) {
  unsigned long long mx = 0, bad = 0;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < count; j += (uint64_t)gridDim.x * kBlock) {
    const unsigned long long v = idx64 ? ((const unsigned long long*)idx)[j] : (unsigned long long)((const uint32_t*)idx)[j];
    mx = v > mx ? v : mx;
    bad += v >= src_len;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = shfl_xor_any(mx, off);
    mx = o > mx ? o : mx;
    bad += shfl_xor_any(bad, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (mx) atomicMax(out2, mx);
    if (bad) atomicAdd(out2 + 1, bad);
  }
}

// ---- keys --------------------------------------------------------------------------------------------------------------------------------
// unsigned: the value; signed: the sign bit flipped; floats: -0.0 as +0.0, then negative values complemented and the others with the sign
// bit set; every NaN the all-ones key.  *nan: the key is a NaN key (descending order leaves it alone)
template <typename T>
__device__ __forceinline__ auto value_key(T v, bool& nan) {
  nan = false;
  if constexpr (std::is_same<T, float>::value) {
    uint32_t b = __builtin_bit_cast(uint32_t, v);
    if (v != v) { nan = true; return 0xFFFFFFFFu; }
    if (b == 0x80000000u) b = 0;
    return (b >> 31) ? ~b : (b | 0x80000000u);
  } else if constexpr (std::is_same<T, double>::value) {
    unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    if (v != v) { nan = true; return ~0ull; }
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  } else if constexpr (sizeof(T) == 8) {
    return std::is_signed<T>::value ? (unsigned long long)v ^ 0x8000000000000000ull : (unsigned long long)v;
  } else {
    using UT = typename std::make_unsigned<T>::type;
    const uint32_t u = (uint32_t)(UT)v;
    return std::is_signed<T>::value ? u ^ (1u << (8 * sizeof(T) - 1)) : u;
  }
}

__global__ __launch_bounds__(kBlock) void attribute_keys_kernel(uint64_t addr, uint64_t stride, uint64_t n, uint32_t ct, uint32_t descending,
                                                                uint32_t* __restrict__ keys32, unsigned long long* __restrict__ keys64, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  cgptr_t p = (cgptr_t)as_global(addr + i * stride);
  dispatch_ct(ct, [&](auto tag) {
    using T = decltype(tag);
    bool nan;
    auto key = value_key<T>(load_un<T>(p), nan);
    if (descending && !nan) key = ~key;
    if constexpr (sizeof(key) == 8) { keys64[i] = key; vals[i] = (uint32_t)i; }
    else keys32[i] = key;
  });
}

__device__ __forceinline__ unsigned long long spread3(unsigned long long x) {  // bit i of the low 21 to bit 3 i
  x &= 0x1FFFFFull;
  x = (x | (x << 32)) & 0x001F00000000FFFFull;
  x = (x | (x << 16)) & 0x001F0000FF0000FFull;
  x = (x | (x << 8)) & 0x100F00F00F00F00Full;
  x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ unsigned long long spread2(unsigned long long x) {  // bit i of the low 32 to bit 2 i
  x &= 0xFFFFFFFFull;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}
// t = (p - min) * inv, two roundings; c = t >= 2^bits ? 2^bits - 1 : t >= 0 ? floor(t) : 0 (a NaN t gives 0)
__device__ __forceinline__ unsigned long long morton_cell(double p, double mn, double inv, double lim) {
  const double d = p - mn;
  const double t = d * inv;
  if (t >= lim) return (unsigned long long)lim - 1ull;
  return t >= 0.0 ? (unsigned long long)t : 0ull;
}

__global__ __launch_bounds__(kBlock) void morton_keys_kernel(Pos pos, uint64_t n, const pstk::MortonGrid g, unsigned long long* __restrict__ sort_keys,
                                                             uint32_t* __restrict__ vals, unsigned long long* __restrict__ out_keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  load_point(pos, i, x, y, z);
  const bool fin = finite(x) && finite(y) && finite(z);
  const double lim = (double)(1ull << g.bits);
  unsigned long long key;
  if (g.dims == 3)
    key = spread3(morton_cell(x, g.min[0], g.inv[0], lim)) | (spread3(morton_cell(y, g.min[1], g.inv[1], lim)) << 1) |
          (spread3(morton_cell(z, g.min[2], g.inv[2], lim)) << 2);
  else
    key = spread2(morton_cell(x, g.min[0], g.inv[0], lim)) | (spread2(morton_cell(y, g.min[1], g.inv[1], lim)) << 1);
  sort_keys[i] = fin ? key : 1ull << (g.dims * g.bits);
  vals[i] = (uint32_t)i;
  if (out_keys) out_keys[i] = fin ? key : 1ull << 63;
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__global__ __launch_bounds__(kBlock) void shuffle_keys_kernel(uint64_t n, uint64_t seed, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  keys[i] = splitmix64(seed ^ i);
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void invert_kernel(const uint32_t* __restrict__ order, uint64_t n, uint32_t* __restrict__ inverse) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = order[j];
  if (i < n) inverse[i] = (uint32_t)j;
}

}  // namespace

namespace pstk {

uint32_t gather_chunk(uint32_t stride) {
  if (stride == 0) return kP;
  const uint32_t fit = (kReorderRecordTileBytes - kReorderTileSlack) / stride;
  return fit < kP ? fit : kP;
}
bool gather_tile_fits(uint32_t stride) { return gather_chunk(stride) >= kReorderMinTileRecords; }

bool gather_points(const GatherArgs& a, bool src_aos, bool dst_aos, bool by_bytes, hipStream_t stream) {
  if (a.count == 0) return true;
  const uint64_t blocks = (a.count + kP - 1) / kP;
  if (blocks > 0x7FFFFFFFull) return false;  // (2^39 points)
  const dim3 grid((unsigned)blocks), block(kBlock);
  if (by_bytes) {
    hipLaunchKernelGGL(gather_bytes_kernel, grid, block, 0, stream, a);
    return launched();
  }
  const uint32_t lds = (src_aos || dst_aos) ? a.chunk * a.stride + kReorderTileSlack : 0;
  if (lds > kReorderRecordTileBytes) return false;
  if (src_aos && dst_aos) hipLaunchKernelGGL((gather_kernel<true, true>), grid, block, lds, stream, a);
  else if (src_aos) hipLaunchKernelGGL((gather_kernel<true, false>), grid, block, lds, stream, a);
  else if (dst_aos) hipLaunchKernelGGL((gather_kernel<false, true>), grid, block, lds, stream, a);
  else hipLaunchKernelGGL((gather_kernel<false, false>), grid, block, 0, stream, a);
  return launched();
}

bool gather_index_check(const void* idx, bool idx64, uint64_t count, uint64_t src_len, unsigned long long* out2, hipStream_t stream) {
  if (count == 0) return true;
  const uint64_t want = (count + kBlock - 1) / kBlock;
  const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(index_check_kernel, dim3(blocks), dim3(kBlock), 0, stream, idx, idx64 ? 1u : 0u, count, src_len, out2);
  return launched();
}

bool reorder_attribute_keys(uint64_t addr, uint64_t stride, uint64_t n, uint32_t ct, bool descending, uint32_t* keys32, unsigned long long* keys64, uint32_t* vals,
                            hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(attribute_keys_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, addr, stride, n, ct, descending ? 1u : 0u, keys32, keys64, vals);
  return launched();
}

bool reorder_morton_keys(const Positions& pos, const MortonGrid& g, unsigned long long* sort_keys, uint32_t* vals, unsigned long long* out_keys, hipStream_t stream) {
  if (pos.n == 0) return true;
  hipLaunchKernelGGL(morton_keys_kernel, dim3(blocks_of(pos.n, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), pos.n, g, sort_keys, vals, out_keys);
  return launched();
}

bool reorder_shuffle_keys(uint64_t n, uint64_t seed, unsigned long long* keys, uint32_t* vals, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(shuffle_keys_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, n, seed, keys, vals);
  return launched();
}

bool reorder_invert(const uint32_t* order, uint64_t n, uint32_t* inverse, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(invert_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, order, n, inverse);
  return launched();
}

}  // namespace pstk
