// M3C2 change detection: signed distances between two indexed clouds along the normals of core points (include/pasture_amd.h, "M3C2 change
// detection"; Lague, Brodu & Leroux 2013).
//
// Definitions (every operation a separately rounded f64 operation).  Core point c, unit normal u = n / sqrt((nx*nx + ny*ny) + nz*nz).  A finite
// point p of a cloud, d = p - c, t = (dx*ux + dy*uy) + dz*uz, w = d - t*u, r2 = (wx*wx + wy*wy) + wz*wz, is a MEMBER of the core point's
// cylinder iff fabs(t) <= L && r2 <= R*R.  Per cloud the kernel reports the number of members, sum t and sum t*t; from the two clouds'
// figures the distance, the level of detection and the significance flag, by the expressions at the end of m3c2_kernel.
//
// Shape.  ONE wave per core point, four core points per workgroup; the core points are taken in the order of their cell keys in the
// reference grid (the API sorts them: neighbouring waves read neighbouring cells) and the results go back to core order.  For each of the
// two clouds in turn the wave walks the (y, z) rows of the cylinder's clamped cell box, 64 rows at a time, one row per lane: the lane
// culls its row (below), and if something is left of it finds the row's key range [row | x0, (row | x1) + 1) in the sorted keys -- a binary
// search for the start, a galloping search from there for the end.  The non-empty ranges of the batch are then tested four at a time, one
// per quarter-wave, sixteen candidates of a range per step; every lane keeps its own count, sum t and sum t*t, and at the end of a cloud the
// wave folds them in a fixed xor tree.  All of it is a fixed function of the core point, the cloud and its grid: two calls give the same bits.
// No floating-point atomics; the only atomics are the integer adds of n_significant (one per workgroup) and of the work counters (one per
// wave, in the WORK instantiation alone).
//
// Which rows and cells may be skipped.  Everything is done in CELL UNITS of the cloud's grid: a = (c - min) / edge, Rc = R / edge,
// Lc = L / edge.  Let S = |ax| + |ay| + |az| + Lc + Rc + (largest dim) + 1: every number the cull computes is at most S in magnitude.
//   the predicate   a member's computed t and r2 differ from the real-number t* = d.u and |w*|, w* = d - t* u, by roundings relative to
//                   |d| <= (L + R)(1 + 2^-50): fl(p - c) is within 2^-53 relative per component, the three products and two sums of t within
//                   8 * 2^-53 |d| together, w within 10 * 2^-53 |d| per component, r2 within 3 * 2^-53 relative.  So a member has
//                   |t*| <= L + 2^-48 (L + R) and |w*| <= R + 2^-48 (L + R).  u is not exactly of unit length; that does not matter: for ANY
//                   u, p = c + t* u + w*, so p lies within |w*| of the point c + t* u of the axis -- the cull below only ever uses this
//                   decomposition, never that w* is perpendicular.
//   the cells       a point's cell number is trunc(fl(fl(p - min) / edge)), two roundings of a value below 2^21: a point of cell k has its
//                   real coordinate (p - min) / edge in [k - 2^-30, k + 1 + 2^-30] (the argument of nn.hip).
//   the units       a, Rc and Lc carry two roundings each, 2^-52 S at the most.
//   the margin      pad = 2^-22 S is added to Rc and to Lc: Rp = Rc + pad, Lp = Lc + pad.  The sum of everything above is below
//                   2^-30 + 2^-46 S <= 2^-29 S, and every expression of the cull adds at most a dozen roundings of numbers up to S, 2^-49 S:
//                   the margin is some 2^7 times what the roundings need, and since S >= 1 it covers the cells' 2^-30 whatever the grid.  It is
//                   relative to the size of the numbers involved, not a length picked by hand: a cloud a million cells across pays a
//                   quarter of a cell.
//   the box         per axis k a member has |p_k - a_k| <= |t*| |u_k| + |w*| <= Lp |u_k| + Rp: the rows walked are those of the cells
//                   [a_k - Lp |u_k| - Rp, a_k + Lp |u_k| + Rp], clamped to the grid; an empty clamp on any axis ends the cloud before any
//                   search (a core point whose cylinder misses the grid costs nothing).
//   a row           (iy, iz): a member in it has, for k = y and z, i_k - 2^-30 <= a_k + t* u_k + w*_k <= i_k + 1 + 2^-30, so
//                   a_k + t* u_k lies in [i_k - Rp, i_k + 1 + Rp]: with u_k != 0 that is an interval of t (the margin sits in the numerator
//                   BEFORE the division, so a small u_k cannot amplify a rounding past it; the quotient's own rounding is 2^-53 |t| <= 2^-53 S),
//                   with u_k == 0 it is a condition on a_k alone.  The two intervals and [-Lp, Lp] are intersected: empty means no member
//                   in the row.  Otherwise x = a_x + t* u_x + w*_x lies within Rp of the two ends' a_x + t u_x: the row's cells x0 .. x1.
//   a cell          a member of cell (ix, iy, iz) is within (sqrt(3) / 2)(1 + 2^-29) of the cell's centre m and within Rc + 2^-48 S of the
//                   axis segment, so m is within Rp + sqrt(3) / 2 of the segment.  The distance from m to the point of the segment at
//                   clamp(v.u, -Lc, Lc), v = m - a, is what is compared (with |u| = 1 +- 2^-51 that point is the nearest one up to
//                   2^-100 S^2 in the squared distance).  The distance to a convex set is convex along the row, so the cells that pass
//                   are contiguous: the range is trimmed from both ends while the end cell fails.  This is "a cell whose distance to
//                   the axis exceeds R plus the cell's half-diagonal is not searched"; it cuts the corners the row test leaves.
//   not finite      every comparison of the cull is written so that a NaN (an S that overflows) keeps the row: the cull can only ever drop
//                   what the argument above covers.
// Hence a cell is skipped only when no point of it can satisfy the ROUNDED predicate: the counts do not depend on the grids, and the sums
// depend on them only through the order of summation.
//
// Cost.  The row test is some sixty flops per row of the BOX, the searches are two chains of dependent loads per row of the CYLINDER: for a
// diagonal normal with L >> R the box has (L / edge)^2 rows and the cylinder L R / edge^2, the first tested 64 at a time by arithmetic alone.
// A cylinder that spans a whole large grid tests every row of it; that is accepted, as nn.hip accepts its far query.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kLanes = pstk::kM3c2LanesPerCore;
constexpr uint32_t kCores = pstk::kM3c2CoresPerBlock;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr double kPadScale = 0x1p-22;
constexpr double kHalfDiagonal = 0.8660254037844388;  // sqrt(3) / 2, rounded up
static_assert(kLanes == 64 && kCores * kLanes == kBlock, "one wave per core point, kBlock threads per workgroup");

using Grid = pstk::NnGrid;
using Cloud = pstk::M3c2Cloud;
using Args = pstk::M3c2Args;

__device__ __forceinline__ double quiet_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }

// first position in keys[lo, hi) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound(const unsigned long long* __restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long k) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the same from `first` on, for a position that is expected close behind it: steps of 8, 16, 32, ... then a binary search of the last step
__device__ __forceinline__ uint32_t gallop_bound(const unsigned long long* __restrict__ keys, uint32_t first, uint32_t nf, unsigned long long k) {
  uint32_t lo = first, hi = first, step = 8;
  while (hi < nf && keys[hi] < k) {
    lo = hi + 1;
    hi = step < nf - hi ? hi + step : nf;
    step <<= 1;
  }
  return lower_bound(keys, lo, hi, k);
}

// the cells [lo, hi] of one axis clamped to [0, dim - 1]; false when none is left.  A NaN keeps the whole axis.
__device__ __forceinline__ bool clamp_cells(double lo, double hi, uint32_t dim, uint32_t& c0, uint32_t& c1) {
  if (lo >= (double)dim || hi < 0.0) return false;
  c0 = lo > 0.0 ? (uint32_t)lo : 0u;                         // (0 < lo < dim: the conversion truncates)
  c1 = hi < (double)(dim - 1) ? (uint32_t)hi : dim - 1;      // (0 <= hi here, or a NaN, which takes dim - 1)
  return true;
}

struct Axis { double a[3], u[3], Rp, Lp, Lc, lim2; };

// true when the centre of cell (ix, iy, iz) is farther than Rp + sqrt(3) / 2 from the axis segment
__device__ __forceinline__ bool cell_far(const Axis& s, uint32_t ix, double my, double mz) {
  const double vx = ((double)ix + 0.5) - s.a[0], vy = my - s.a[1], vz = mz - s.a[2];
  double t = (vx * s.u[0] + vy * s.u[1]) + vz * s.u[2];
  t = t < -s.Lc ? -s.Lc : (t > s.Lc ? s.Lc : t);
  const double ex = vx - t * s.u[0], ey = vy - t * s.u[1], ez = vz - t * s.u[2];
  return (ex * ex + ey * ey) + ez * ez > s.lim2;
}

// the cells x0 .. x1 of row (iy, iz) that can hold a member; false: none
__device__ __forceinline__ bool row_cells(const Axis& s, uint32_t iy, uint32_t iz, uint32_t dimx, uint32_t& x0, uint32_t& x1) {
  double ta = -s.Lp, tb = s.Lp;
  const double cell[2] = {(double)iy, (double)iz};
#pragma unroll
  for (int k = 1; k <= 2; ++k) {
    const double lo = cell[k - 1] - s.Rp, hi = (cell[k - 1] + 1.0) + s.Rp;
    if (s.u[k] == 0.0) {
      if (s.a[k] < lo || s.a[k] > hi) return false;
    } else {
      double t0 = (lo - s.a[k]) / s.u[k], t1 = (hi - s.a[k]) / s.u[k];
      if (t0 > t1) { const double x = t0; t0 = t1; t1 = x; }
      if (t0 > ta) ta = t0;
      if (t1 < tb) tb = t1;
    }
  }
  if (ta > tb) return false;
  const double xa = s.a[0] + ta * s.u[0], xb = s.a[0] + tb * s.u[0];
  const double xlo = (xa < xb ? xa : xb) - s.Rp, xhi = (xa < xb ? xb : xa) + s.Rp;
  if (!clamp_cells(xlo, xhi, dimx, x0, x1)) return false;
  const double my = cell[0] + 0.5, mz = cell[1] + 0.5;
  while (x0 < x1 && cell_far(s, x0, my, mz)) ++x0;
  while (x1 > x0 && cell_far(s, x1, my, mz)) --x1;
  return !(x0 == x1 && cell_far(s, x0, my, mz));
}

struct Tally { uint32_t n; double st, stt; };
struct Work { unsigned long long rows, candidates, members; };

// the members of the cylinder (c, u, R, L) in one cloud: the wave's folded count and sums, the same in every lane
template <bool WORK>
__device__ __forceinline__ Tally cylinder(const Cloud& cl, double cx, double cy, double cz, double ux, double uy, double uz, double R, double L, double RR, uint32_t lane,
                                          Work& work) {
  Tally sum{0u, 0.0, 0.0};
  if (cl.nf == 0) return sum;
  const Grid& g = cl.g;
  const uint32_t nf = cl.nf;
  const unsigned long long* __restrict__ keys = cl.keys;
  const double* __restrict__ xs = cl.xs;
  const double* __restrict__ ys = cl.ys;
  const double* __restrict__ zs = cl.zs;
  Axis s;
  s.a[0] = (cx - g.min[0]) / g.edge; s.a[1] = (cy - g.min[1]) / g.edge; s.a[2] = (cz - g.min[2]) / g.edge;
  s.u[0] = ux; s.u[1] = uy; s.u[2] = uz;
  const double Rc = R / g.edge;
  s.Lc = L / g.edge;
  const uint32_t dim_max = max(g.dim[0], max(g.dim[1], g.dim[2]));
  const double S = (((__builtin_fabs(s.a[0]) + __builtin_fabs(s.a[1])) + __builtin_fabs(s.a[2])) + (s.Lc + Rc)) + ((double)dim_max + 1.0);
  const double pad = S * kPadScale;
  s.Rp = Rc + pad;
  s.Lp = s.Lc + pad;
  const double lim = s.Rp + kHalfDiagonal;
  s.lim2 = lim * lim;
  uint32_t b0[3], b1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ext = s.Lp * __builtin_fabs(s.u[k]) + s.Rp;
    if (!clamp_cells(s.a[k] - ext, s.a[k] + ext, g.dim[k], b0[k], b1[k])) return sum;  // (wave-uniform)
  }
  const uint32_t ny = b1[1] - b0[1] + 1, nz = b1[2] - b0[2] + 1;
  const uint32_t bx = g.bits[0], by = g.bits[1];
  const uint32_t quarter = lane >> 4, sub = lane & 15;
  // the batch's first row as (y, z) offsets into the box; 64 rows further every round
  uint32_t oy = 0, oz = 0;
#pragma unroll 1
  while (oz < nz) {
    uint32_t first = 0, last = 0;
    {
      const uint32_t ry = oy + lane;  // (oy < ny <= 2^21: no overflow)
      const uint32_t rz = oz + ry / ny;
      if (rz < nz) {
        const uint32_t iy = b0[1] + ry % ny, iz = b0[2] + rz;
        uint32_t x0, x1;
        if (row_cells(s, iy, iz, g.dim[0], x0, x1)) {
          const unsigned long long row = ((unsigned long long)iz << (bx + by)) | ((unsigned long long)iy << bx);
          first = lower_bound(keys, 0, nf, row | x0);
          last = gallop_bound(keys, first, nf, (row | x1) + 1);
          if constexpr (WORK) work.rows += 1;
        }
      }
    }
    unsigned long long todo = __ballot(first < last);
#pragma unroll 1
    while (todo) {  // (wave-uniform) the next four non-empty ranges, one per quarter-wave
      int src = 64;
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        const int bit = todo ? __builtin_ctzll(todo) : 64;
        todo = todo ? todo & (todo - 1) : 0;
        src = quarter == q ? bit : src;
      }
      const uint32_t f = (uint32_t)__shfl((int)first, src & 63, 64), l = (uint32_t)__shfl((int)last, src & 63, 64);
      uint32_t c = src < 64 ? f + sub : 0u;
      const uint32_t end = src < 64 ? l : 0u;
#pragma unroll 1
      while (c < end) {
        const double dx = xs[c] - cx, dy = ys[c] - cy, dz = zs[c] - cz;
        const double t = (dx * ux + dy * uy) + dz * uz;
        const double wx = dx - t * ux, wy = dy - t * uy, wz = dz - t * uz;
        const double r2 = (wx * wx + wy * wy) + wz * wz;
        if (__builtin_fabs(t) <= L && r2 <= RR) {
          sum.n += 1;
          sum.st = sum.st + t;
          sum.stt = sum.stt + t * t;
        }
        if constexpr (WORK) work.candidates += 1;
        c += 16;
      }
    }
    oy += 64;
    oz += oy / ny;
    oy %= ny;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sum.n = sum.n + shfl_xor_any(sum.n, off);
    sum.st = sum.st + shfl_xor_any(sum.st, off);
    sum.stt = sum.stt + shfl_xor_any(sum.stt, off);
  }
  if constexpr (WORK) work.members += lane == 0 ? sum.n : 0u;
  return sum;
}

template <bool WORK>
__global__ __launch_bounds__(kBlock, 4) void m3c2_kernel(Args p) {
  __shared__ uint32_t flagged[kCores];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t s = (uint64_t)blockIdx.x * kCores + wave;
  uint32_t significant = 0;
  if (s < p.n) {  // (wave-uniform)
    const uint32_t i = p.order ? __builtin_amdgcn_readfirstlane(p.order[s]) : (uint32_t)s;
    double cx, cy, cz;
    load_point(Pos{(cgptr_t)p.core_base, p.core_stride}, i, cx, cy, cz);
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    bool valid = finite(cx) && finite(cy) && finite(cz);
    if (p.normals) {
      n0 = p.normals[3 * (uint64_t)i]; n1 = p.normals[3 * (uint64_t)i + 1]; n2 = p.normals[3 * (uint64_t)i + 2];
    } else {
      const uint32_t a = (valid && p.at && p.nx) ? p.at[i] : kNone;
      if (a != kNone) { n0 = p.nx[a]; n1 = p.ny[a]; n2 = p.nz[a]; }
      else valid = false;
    }
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    valid = valid && finite(n0) && finite(n1) && finite(n2) && nn != 0.0 && finite(nn);
    double ux = quiet_nan(), uy = quiet_nan(), uz = quiet_nan();
    Tally t1{0u, 0.0, 0.0}, t2{0u, 0.0, 0.0};
    Work work{0, 0, 0};
    if (valid) {  // (wave-uniform)
      const double len = __builtin_sqrt(nn);
      ux = n0 / len; uy = n1 / len; uz = n2 / len;
      // (the sign bits are flipped by a mask, not under a branch)
      const bool down = uz < 0.0 || (uz == 0.0 && (uy < 0.0 || (uy == 0.0 && ux < 0.0)));
      const unsigned long long turn = ((p.flags & 1u) && down) ? 0x8000000000000000ull : 0ull;
      ux = __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, ux) ^ turn);
      uy = __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, uy) ^ turn);
      uz = __builtin_bit_cast(double, __builtin_bit_cast(unsigned long long, uz) ^ turn);
#pragma unroll 1
      for (int X = 0; X < 2; ++X) {  // the same body serves both clouds
        const Tally t = cylinder<WORK>(p.cloud[X], cx, cy, cz, ux, uy, uz, p.radius, p.max_depth, p.radius2, lane, work);
        if (X == 0) t1 = t; else t2 = t;
      }
    }
    // the results: the expressions of the header, in its order of operations
    double distance = quiet_nan(), lod = quiet_nan();
    if (valid && t1.n >= p.min_points && t2.n >= p.min_points) {
      const double m1 = (double)t1.n, m2 = (double)t2.n;
      const double mean1 = t1.st / m1, mean2 = t2.st / m2;
      distance = mean2 - mean1;
      if (t1.n >= 2 && t2.n >= 2) {
        const double q1 = t1.stt - (t1.st * t1.st) / m1, q2 = t2.stt - (t2.st * t2.st) / m2;
        const double var1 = (q1 > 0.0 ? q1 : 0.0) / (double)(t1.n - 1), var2 = (q2 > 0.0 ? q2 : 0.0) / (double)(t2.n - 1);
        lod = 1.96 * (__builtin_sqrt(var1 / m1 + var2 / m2) + p.registration_error);
      }
    }
    significant = __builtin_fabs(distance) > lod ? 1u : 0u;  // (false for a NaN on either side)
    if (lane == 0) {
      if (p.distance) p.distance[i] = distance;
      if (p.lod) p.lod[i] = lod;
      if (p.significant) p.significant[i] = (uint8_t)significant;
      if (p.counts) { p.counts[2 * (uint64_t)i] = t1.n; p.counts[2 * (uint64_t)i + 1] = t2.n; }
      if (p.sums) {
        double* o = p.sums + 4 * (uint64_t)i;
        o[0] = t1.st; o[1] = t1.stt; o[2] = t2.st; o[3] = t2.stt;
      }
      if (p.unit_normals) {
        double* o = p.unit_normals + 3 * (uint64_t)i;
        o[0] = ux; o[1] = uy; o[2] = uz;
      }
    }
    if constexpr (WORK) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        work.rows += shfl_xor_any(work.rows, off);
        work.candidates += shfl_xor_any(work.candidates, off);
        work.members += shfl_xor_any(work.members, off);
      }
      if (lane == 0) {
        if (work.rows) atomicAdd(p.work, work.rows);
        if (work.candidates) atomicAdd(p.work + 1, work.candidates);
        if (work.members) atomicAdd(p.work + 2, work.members);
      }
    }
  }
  if (lane == 0) flagged[wave] = significant;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCores; ++w) total += flagged[w];
    if (total) atomicAdd(p.n_significant, (unsigned long long)total);
  }
}

}  // namespace

namespace pstk {

bool m3c2_run(const M3c2Args& a, hipStream_t stream) {
  if (hipMemsetAsync(a.n_significant, 0, sizeof(unsigned long long), stream) != hipSuccess) return false;
  if (a.work && hipMemsetAsync(a.work, 0, 3 * sizeof(unsigned long long), stream) != hipSuccess) return false;
  if (a.n == 0) return true;
  const unsigned blocks = blocks_of(a.n, kCores);
  if (a.work) hipLaunchKernelGGL(m3c2_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL(m3c2_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, a);
  return launched();
}

}  // namespace pstk
