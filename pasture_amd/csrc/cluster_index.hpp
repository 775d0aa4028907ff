// The host side of the cluster index, shared by the drivers of the neighbour-based algorithms (clusters_api.cpp, dbscan_api.cpp,
// sample_api.cpp, nn_api.cpp; the bounds also by pmf_api.cpp, hag_api.cpp, raster_api.cpp, quantiles_api.cpp and reorder_api.cpp).  Its
// counterpart for 32-bit keys over a 2-D grid or over labels is the dense directory (dense_directory.hpp).
//
// "The cluster index" of a cloud: the AABB of its finite points, read back -> (host: a ClusterGrid, cluster_grid.hpp) -> cluster_keys -> the
// 64-bit pair sort on bits[0] + bits[1] + bits[2] + 1 bits, which puts the nf finite points in cell order in front of the others -> nn_gather:
// their positions in that order.  The kernels that walk it share their device code in grid_index_device.hpp.
#pragma once
#include <utility>

#include "device_sort.hpp"
#include "runtime.hpp"

namespace pst {

// ---- bounds, read back: each launches into the regions the caller names, copies the record, synchronises ONCE and returns plain doubles ------

// the AABB of the points whose three components are finite, and their number (count == 0: min and max mean nothing)
struct FiniteBounds { double min[3], max[3]; uint64_t count; };

// through cluster_bounds (block folds, then integer atomics on the ordered encoding); rec: 256 bytes
inline FiniteBounds finite_bounds(const pstk::Positions& pos, pstk::ClusterRecord* rec, hipStream_t s, const std::string& who) {
  if (!pstk::cluster_bounds(pos, rec, s)) throw hip_failure(who + ": bounds launch failed: ");
  pstk::ClusterRecord r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  FiniteBounds b{};
  for (int a = 0; a < 3; ++a) {
    b.min[a] = pstk::cluster_decode_ordered(r.min_ordered[a]);
    b.max[a] = pstk::cluster_decode_ordered(r.max_ordered[a]);
  }
  b.count = r.finite_count;
  return b;
}

// through sample_bounds (block partials, then one folding workgroup; no atomics); partials: sample_bounds_partials_bytes(n), rec: 256 bytes
inline FiniteBounds finite_bounds_folded(const pstk::Positions& pos, void* partials, pstk::SampleBounds* rec, hipStream_t s, const std::string& who) {
  if (!pstk::sample_bounds(pos, partials, rec, s)) throw hip_failure(who + ": bounds launch failed: ");
  pstk::SampleBounds r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  return FiniteBounds{{r.min[0], r.min[1], r.min[2]}, {r.max[0], r.max[1], r.max[2]}, r.count};
}

// In x and y, through hag_bounds, of the finite points whose mask byte is not zero (mask == nullptr: of every finite point).  The block
// partials are needed before the caller's grid -- and with it the size of its scratch -- is known: they live in a small block of their own.
inline pstk::HagBounds finite_bounds_2d(const pstk::Positions& pos, const uint8_t* mask, hipStream_t s, const char* who) {
  ScratchLayout layout;
  const size_t off_partials = layout.add(pstk::hag_bounds_partials_bytes(pos.n)), off_rec = layout.add(sizeof(pstk::HagBounds));
  Scratch block(layout, s, who);
  pstk::HagBounds* rec = block.at<pstk::HagBounds>(off_rec);
  if (!pstk::hag_bounds(pos, mask, block.at<void>(off_partials), rec, s)) throw hip_failure(std::string(who) + ": bounds launch failed: ");
  pstk::HagBounds r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  return r;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------------------------------

// cluster_grid.hpp's grid of a search within `tolerance` over these bounds
inline pstk::ClusterGrid cluster_grid_over(const FiniteBounds& b, double tolerance, const std::string& who) {
  pstk::ClusterGrid g{};
  if (!pstk::cluster_grid_for_tolerance(b.min, b.max, tolerance, &g)) throw Error(PST_ERR_UNSUPPORTED, who + ": the extent of the finite points overflows f64");
  return g;
}

// ---- keys and sort -----------------------------------------------------------------------------------------------------------------------------

// keys_a[i] = cell key of point i (all ones: not finite), vals_a[i] = i; then the pairs sorted into keys_b | order, stable.  tmp: what
// sort_pairs_u64 asks for pos.n pairs.
inline void cluster_sorted_keys(const pstk::Positions& pos, const pstk::ClusterGrid& grid, uint64_t* keys_a, uint64_t* keys_b, uint32_t* vals_a, uint32_t* order, void* tmp,
                                size_t tmp_bytes, hipStream_t s, const std::string& who) {
  if (!pstk::cluster_keys(pos, grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure(who + ": key launch failed: ");
  PST_HIP_CHECK(pstk::sort_pairs_u64(tmp, tmp_bytes, keys_a, keys_b, vals_a, order, pos.n, grid.bits[0] + grid.bits[1] + grid.bits[2] + 1, s));
}

// The seven regions of the index in a call's one block of scratch, for n points: b4 = up256((n + 1) * 4) bytes hold a 4-byte array with one
// element to spare, and an 8-byte array's room is exactly two of them (the callers reuse the dead regions as such halves):
//   keys_a (2 b4)      unsorted keys     dead after the sort
//   keys_b (2 b4)      sorted keys
//   vals_a (b4)        unsorted indices  dead after the sort
//   order  (b4)        buffer index of sorted position s
//   xs, ys, zs (2 b4)  sorted positions of the nf finite points
struct ClusterIndex {
  size_t b4 = 0, off[7] = {};
  uint64_t *keys_a = nullptr, *keys_b = nullptr;
  uint32_t *vals_a = nullptr, *order = nullptr;
  double *xs = nullptr, *ys = nullptr, *zs = nullptr;

  void carve(ScratchLayout& layout, size_t n) {
    b4 = up256((n + 1) * 4);
    const size_t bytes[7] = {2 * b4, 2 * b4, b4, b4, 2 * b4, 2 * b4, 2 * b4};
    for (int i = 0; i < 7; ++i) off[i] = layout.add(bytes[i]);
  }
  void bind(Scratch& scratch) {
    keys_a = scratch.at<uint64_t>(off[0]);
    keys_b = scratch.at<uint64_t>(off[1]);
    vals_a = scratch.at<uint32_t>(off[2]);
    order = scratch.at<uint32_t>(off[3]);
    xs = scratch.at<double>(off[4]);
    ys = scratch.at<double>(off[5]);
    zs = scratch.at<double>(off[6]);
  }
  // an 8-byte region as two 4-byte arrays
  std::pair<uint32_t*, uint32_t*> halves(void* p) const { return {(uint32_t*)p, (uint32_t*)((uint8_t*)p + b4)}; }
  const unsigned long long* sorted_keys() const { return (const unsigned long long*)keys_b; }
  // keys -> sort -> (gather: the positions of the nf finite points; cluster_components gathers itself)
  void build(const pstk::Positions& pos, const pstk::ClusterGrid& grid, uint32_t nf, void* tmp, size_t tmp_bytes, hipStream_t s, const std::string& who, bool gather) {
    cluster_sorted_keys(pos, grid, keys_a, keys_b, vals_a, order, tmp, tmp_bytes, s, who);
    if (gather && !pstk::nn_gather(pos, order, nf, xs, ys, zs, s)) throw hip_failure(who + ": gather launch failed: ");
  }
};

}  // namespace pst
