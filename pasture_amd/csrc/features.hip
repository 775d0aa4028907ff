// Per-point geometric features from the eigenvalues of the neighbourhood covariance, over neighbour lists uint32 [n][k] in device memory (the
// lists of the kNN search, or a caller's).  The definition is in include/pasture_amd.h ("Geometric features"); tests/features_ref.py restates
// it in numpy.  Every operation is a separately rounded f64 operation (-ffp-contract=off) except cbrt and log.
//
// The kernel maps the lists flat, as outlier_distance_kernel does: a workgroup owns P = features_points_per_block(k) consecutive points, that is
// P * k consecutive list elements, and walks them kFeaturesThreads at a time -- element e = q * k + t is read by thread e mod kFeaturesThreads
// of its pass, so the index reads are coalesced.  That thread decides the slot's validity (index in range, neighbour and query finite, distance
// within max_distance) and does the one random 24-byte gather; it stages x, y, z into an LDS tile, or a NaN in x where the slot is not valid
// (a valid slot's x is finite).  A point's row is 3 * k doubles padded to an odd number.  After the barrier one lane per point walks its row
// twice in slot order (centroid, covariance), runs the cyclic Jacobi sweeps on named registers -- the three (p, q) pairs are written out, no
// array is indexed by a runtime value -- and writes each requested plane with lane = point, consecutive addresses per plane.
#include "positions_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kThreads = pstk::kFeaturesThreads;
static_assert(kThreads == kBlock, "the feature kernel is written for one kBlock workgroup");

__device__ __forceinline__ double canonical_nan() { return __builtin_bit_cast(double, 0x7FF8000000000000ull); }

// One Jacobi rotation that annihilates a_pq; r is the third index.  Steps 1 - 4 of the definition.
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p, double& v1q,
                                       double& v2p, double& v2q) {
  const double g = __builtin_fabs(apq);
  if (g != 0.0 && __builtin_fabs(app) + g == __builtin_fabs(app) && __builtin_fabs(aqq) + g == __builtin_fabs(aqq)) apq = 0.0;
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  double p = v0p, q = v0q;
  v0p = c * p - s * q; v0q = s * p + c * q;
  p = v1p; q = v1q;
  v1p = c * p - s * q; v1q = s * p + c * q;
  p = v2p; q = v2q;
  v2p = c * p - s * q; v2q = s * p + c * q;
}

// stable descending order: the pair is exchanged only where the later value is strictly larger
__device__ __forceinline__ void order_pair(double& la, double& lb, double& a0, double& a1, double& a2, double& b0, double& b1, double& b2) {
  if (lb > la) {
    double t = la; la = lb; lb = t;
    t = a0; a0 = b0; b0 = t;
    t = a1; a1 = b1; b1 = t;
    t = a2; a2 = b2; b2 = t;
  }
}

// normals point up: negated iff z < 0, or z == 0 and y < 0, or z == 0 and y == 0 and x < 0
// (one flag and three selects, no short-circuit branches)
__device__ __forceinline__ void orient(double& x, double& y, double& z) {
  const bool flip = (z < 0.0) | ((z == 0.0) & ((y < 0.0) | ((y == 0.0) & (x < 0.0))));
  x = flip ? -x : x;
  y = flip ? -y : y;
  z = flip ? -z : z;
}

__device__ __forceinline__ void store3(double* __restrict__ dst, uint64_t q, double x, double y, double z) {
  dst[q * 3] = x; dst[q * 3 + 1] = y; dst[q * 3 + 2] = z;
}

__global__ __launch_bounds__(kThreads) void features_kernel(Pos pos, uint64_t n, uint32_t k, uint32_t P, const uint32_t* __restrict__ knn, double max_distance,
                                                            uint32_t features, double* __restrict__ out, double* __restrict__ normals,
                                                            double* __restrict__ directions) {
  extern __shared__ double tile[];  // P rows of (3 * k) | 1 doubles
  const uint64_t q0 = (uint64_t)blockIdx.x * P;
  const uint32_t points = (uint32_t)(n - q0 < P ? n - q0 : P);
  const uint32_t elements = points * k, row = (3u * k) | 1u;
  const uint64_t e0 = q0 * k;
  for (uint32_t l = threadIdx.x; l < elements; l += kThreads) {
    const uint32_t p = l / k, t = l - p * k;
    const uint32_t j = knn[e0 + l];
    double x = canonical_nan(), y = 0.0, z = 0.0;
    if (j < n) {
      double qx, qy, qz, px, py, pz;
      load_point(pos, q0 + p, qx, qy, qz);
      load_point(pos, j, px, py, pz);
      const double dx = px - qx, dy = py - qy, dz = pz - qz;
      const double d = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
      if (finite(qx) && finite(qy) && finite(qz) && finite(px) && finite(py) && finite(pz) && d <= max_distance) { x = px; y = py; z = pz; }
    }
    double* s = tile + p * row + 3u * t;
    s[0] = x; s[1] = y; s[2] = z;
  }
  __syncthreads();
  if (threadIdx.x >= points) return;
  const uint64_t q = q0 + threadIdx.x;
  const double* r = tile + threadIdx.x * row;

  // centroid: the valid slots left to right, starting from the first valid one
  uint32_t m = 0;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  for (uint32_t t = 0; t < k; ++t) {
    const double x = r[3 * t], y = r[3 * t + 1], z = r[3 * t + 2];
    if (finite(x)) {
      if (m == 0) { cx = x; cy = y; cz = z; }
      else { cx = cx + x; cy = cy + y; cz = cz + z; }
      ++m;
    }
  }
  const double md = (double)m;
  cx = cx / md; cy = cy / md; cz = cz / md;
  // population covariance, the same way
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
  bool first = true;
  for (uint32_t t = 0; t < k; ++t) {
    const double x = r[3 * t];
    if (finite(x)) {
      const double dx = x - cx, dy = r[3 * t + 1] - cy, dz = r[3 * t + 2] - cz;
      const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
      if (first) { a00 = xx; a01 = xy; a02 = xz; a11 = yy; a12 = yz; a22 = zz; first = false; }
      else { a00 = a00 + xx; a01 = a01 + xy; a02 = a02 + xz; a11 = a11 + yy; a12 = a12 + yz; a22 = a22 + zz; }
    }
  }
  a00 = a00 / md; a01 = a01 / md; a02 = a02 / md; a11 = a11 / md; a12 = a12 / md; a22 = a22 / md;

  // scale: the largest absolute entry; it is not finite iff an entry is not (a NaN entry would slip through a chain of comparisons)
  const bool entries_finite = finite(a00) && finite(a01) && finite(a02) && finite(a11) && finite(a12) && finite(a22);
  double scale = __builtin_fabs(a00);
  scale = __builtin_fabs(a01) > scale ? __builtin_fabs(a01) : scale;
  scale = __builtin_fabs(a02) > scale ? __builtin_fabs(a02) : scale;
  scale = __builtin_fabs(a11) > scale ? __builtin_fabs(a11) : scale;
  scale = __builtin_fabs(a12) > scale ? __builtin_fabs(a12) : scale;
  scale = __builtin_fabs(a22) > scale ? __builtin_fabs(a22) : scale;

  const double nan = canonical_nan();
  double l1 = nan, l2 = nan, l3 = nan, sum = nan;
  double lin = nan, pla = nan, sca = nan, ani = nan, sv = nan, ver = nan, omni = nan, ent = nan;
  double n0 = nan, n1 = nan, n2 = nan, d0 = nan, d1 = nan, d2 = nan;
  if (m >= 3 && entries_finite) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    if (scale == 0.0) {
      l1 = 0.0; l2 = 0.0; l3 = 0.0;
    } else {
      a00 = a00 / scale; a01 = a01 / scale; a02 = a02 / scale; a11 = a11 / scale; a12 = a12 / scale; a22 = a22 / scale;
      for (int sweep = 0; sweep < 10; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
        rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
        rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
      }
      l1 = a00 * scale; l2 = a11 * scale; l3 = a22 * scale;
    }
    // columns of V travel with their eigenvalues
    order_pair(l1, l2, v00, v10, v20, v01, v11, v21);
    order_pair(l2, l3, v01, v11, v21, v02, v12, v22);
    order_pair(l1, l2, v00, v10, v20, v01, v11, v21);
    l1 = l1 > 0.0 ? l1 : 0.0;
    l2 = l2 > 0.0 ? l2 : 0.0;
    l3 = l3 > 0.0 ? l3 : 0.0;
    sum = (l1 + l2) + l3;
    if (l1 != 0.0) {
      d0 = v00; d1 = v10; d2 = v20;
      n0 = v02; n1 = v12; n2 = v22;
      orient(d0, d1, d2);
      orient(n0, n1, n2);
      lin = (l1 - l2) / l1;
      pla = (l2 - l3) / l1;
      sca = l3 / l1;
      ani = (l1 - l3) / l1;
      sv = l3 / sum;
      ver = 1.0 - __builtin_fabs(n2);
      const double e1 = l1 / sum, e2 = l2 / sum, e3 = l3 / sum;
      if (features & PST_FEATURE_OMNIVARIANCE) omni = cbrt((e1 * e2) * e3);
      if (features & PST_FEATURE_EIGENENTROPY) {
        double h = 0.0;
        if (e1 > 0.0) h = h - e1 * log(e1);
        if (e2 > 0.0) h = h - e2 * log(e2);
        if (e3 > 0.0) h = h - e3 * log(e3);
        ent = h;
      }
    }
  }

  if (out) {
    double* o = out + q;  // one plane per set bit, ascending
    if (features & PST_FEATURE_EIGENVALUE_1) { *o = l1; o += n; }
    if (features & PST_FEATURE_EIGENVALUE_2) { *o = l2; o += n; }
    if (features & PST_FEATURE_EIGENVALUE_3) { *o = l3; o += n; }
    if (features & PST_FEATURE_LINEARITY) { *o = lin; o += n; }
    if (features & PST_FEATURE_PLANARITY) { *o = pla; o += n; }
    if (features & PST_FEATURE_SCATTERING) { *o = sca; o += n; }
    if (features & PST_FEATURE_ANISOTROPY) { *o = ani; o += n; }
    if (features & PST_FEATURE_SURFACE_VARIATION) { *o = sv; o += n; }
    if (features & PST_FEATURE_EIGENVALUE_SUM) { *o = sum; o += n; }
    if (features & PST_FEATURE_VERTICALITY) { *o = ver; o += n; }
    if (features & PST_FEATURE_OMNIVARIANCE) { *o = omni; o += n; }
    if (features & PST_FEATURE_EIGENENTROPY) { *o = ent; o += n; }
    if (features & PST_FEATURE_COUNT) { *o = md; }
  }
  if (normals) store3(normals, q, n0, n1, n2);
  if (directions) store3(directions, q, d0, d1, d2);
}

}  // namespace

namespace pstk {

uint32_t features_points_per_block(uint32_t k) { return k <= 8 ? 256u : k <= 16 ? 128u : k <= 32 ? 64u : 32u; }

bool geometric_features(const Positions& pos, uint32_t k, const uint32_t* knn_dev, double max_distance, uint32_t features, double* out_dev, double* normals_dev,
                        double* directions_dev, hipStream_t stream) {
  if (pos.n == 0) return true;
  const uint32_t P = features_points_per_block(k);
  const size_t lds = (size_t)P * ((3u * k) | 1u) * sizeof(double);  // at most 51 200 bytes (k = 8, 16): three workgroups per compute unit
  hipLaunchKernelGGL(features_kernel, dim3(blocks_of(pos.n, P)), dim3(kThreads), lds, stream, pos_of(pos), pos.n, k, P, knn_dev, max_distance, features, out_dev,
                     normals_dev, directions_dev);
  return launched();
}

}  // namespace pstk
