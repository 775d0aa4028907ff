// Reading Vec3f64 positions in a kernel, and the launchers' two host helpers: shared by ransac.hip, outliers.hip and clusters.hip.
#pragma once
#include "device_common.hpp"
#include "kernels.hpp"

namespace pstd {

constexpr double kInf = __builtin_huge_val();

// pstk::Positions as the kernels take it, by value (16 bytes: the number of points stays a kernel argument of its own)
struct Pos { cgptr_t base; uint64_t stride; };
inline Pos pos_of(const pstk::Positions& p) { return Pos{(cgptr_t)p.base, p.stride}; }
__device__ __forceinline__ void load_point(const Pos& p, uint64_t i, double& x, double& y, double& z) {
  cgptr_t q = p.base + i * p.stride;  // a packed record puts the Vec3f64 at any byte offset
  x = load_un<double>(q); y = load_un<double>(q + 8); z = load_un<double>(q + 16);
}
__device__ __forceinline__ bool finite(double v) { return __builtin_fabs(v) < kInf; }  // false for a NaN

// order-preserving map of the finite doubles onto unsigned integers (-0.0 below +0.0), and back: what the integer atomicMin / atomicMax of
// clusters.hip (the AABB) and pmf.hip (the AABB, the min-z raster) fold
__host__ __device__ __forceinline__ unsigned long long ordered(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double decode_ordered(unsigned long long v) {
  const unsigned long long u = (v >> 63) ? (v & 0x7FFFFFFFFFFFFFFFull) : ~v;
  return __builtin_bit_cast(double, u);
}

inline unsigned blocks_of(uint64_t n, uint32_t per) { return (unsigned)((n + per - 1) / per); }
inline bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace pstd
