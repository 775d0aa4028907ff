// pst_dbscan / pst_dbscan_kernel_shape / pst_dbscan_phase_times: argument checks, the grid, the scratch layout and the order of the launches
// of dbscan.hip (where the pipeline is laid out; the definitions are in include/pasture_amd.h, the argument for the grid's margin at the head
// of clusters.hip).
#include <cmath>
#include <cstring>
#include <utility>

#include "device_sort.hpp"
#include "runtime.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};

// PST_DBSCAN_TIMES=1: stream events around the four phases of every call (tools/bench_dbscan.py reads them through pst_dbscan_phase_times)
struct PhaseEvents {
  hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool on;
  PhaseEvents() {
    static const bool wanted = env_nonzero("PST_DBSCAN_TIMES");
    on = wanted;
    if (on)
      for (auto& ev : e) PST_HIP_CHECK(hipEventCreate(&ev));
  }
  ~PhaseEvents() {
    for (auto ev : e)
      if (ev) (void)hipEventDestroy(ev);
  }
  void mark(int i, hipStream_t s) {
    if (on) PST_HIP_CHECK(hipEventRecord(e[i], s));
  }
  void read() {  // after the stream has been synchronised
    for (int i = 0; i < 4; ++i) {
      float ms = 0.f;
      if (on) PST_HIP_CHECK(hipEventElapsedTime(&ms, e[i], e[i + 1]));
      t_phase_ms[i] = ms;
    }
  }
};

}  // namespace

extern "C" {

int pst_dbscan_kernel_shape(uint32_t* points_per_block) {
  if (points_per_block) *points_per_block = pstk::kDbscanPointsPerBlock;
  return PST_OK;
}

int pst_dbscan_phase_times(double ms[4]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_dbscan(const pst_buffer* b, double eps, uint64_t min_points, uint32_t* labels, uint8_t* core, uint32_t memkind, uint64_t* sizes, size_t sizes_capacity,
               uint64_t counts[3]) {
  PST_API_BEGIN
  const std::string who = "pst_dbscan";
  not_null(b, "buffer");
  not_null(labels, "labels");
  not_null(counts, "counts");
  if (memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid labels memory kind");
  const double e2 = eps * eps;
  if (!std::isfinite(eps) || !(eps > 0.0) || !std::isnormal(e2)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": eps must be finite and positive, and its square a normal number");
  if (min_points == 0) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": min_points must be at least 1");
  const Member* pm = position_vec3f64(*b);
  if (!pm) throw Error(PST_ERR_MISSING_ATTRIBUTE, "Attribute not found in PointLayout of buffer");
  ensure_device();
  if (b->len >= 0xFFFFFFF0ull) throw Error(PST_ERR_UNSUPPORTED, who + ": more than 2^32 - 17 points per call");
  counts[0] = counts[1] = counts[2] = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points: no clusters, no label and no core byte to write

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, *pm);
  const bool on_device = memkind == PST_MEM_DEVICE;

  // One block of scratch, the clusters' plus n bytes of core flags.  The sort's input pair is dead once the sort has run, the sorted keys and
  // positions once the border kernel has; the bookkeeping lives in them:
  //   keys_a (8n)      unsorted keys            -> size | smallest member, per root (from the border kernel on)
  //   keys_b (8n)      sorted keys              -> the clusters' list (keys | roots), sorted
  //   vals_a (4n)      unsorted indices         -> root of every sorted point
  //   order  (4n)      buffer index of sorted position s, to the end
  //   xs (8n)          sorted positions         -> the clusters' list (keys | roots), unsorted
  //   ys (8n)                                   -> rank of every root
  //   zs (8n)                                   -> root of the flagged point | flags (n + 1)
  //   parent (4n), core (n), offsets (8(n + 1): the scan; then the sizes), record, counts, sort / scan scratch, labels and core in buffer order
  //   (host outputs only)
  size_t sort64_bytes = 0, sort32_bytes = 0, scan_bytes = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort64_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort32_bytes, nullptr, nullptr, nullptr, nullptr, n, 32, s));
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
  const size_t tmp_bytes = std::max(sort64_bytes, std::max(sort32_bytes, scan_bytes));
  const size_t b4 = up256((n + 1) * 4), b8 = 2 * b4;  // an 8-byte array's room is exactly two 4-byte arrays' (the halves are used as such)
  const auto halves = [b4](void* p) { return std::pair<uint32_t*, uint32_t*>{(uint32_t*)p, (uint32_t*)((uint8_t*)p + b4)}; };
  ScratchLayout layout;
  const size_t off_keys_a = layout.add(b8), off_keys_b = layout.add(b8), off_vals_a = layout.add(b4), off_order = layout.add(b4);
  const size_t off_xs = layout.add(b8), off_ys = layout.add(b8), off_zs = layout.add(b8), off_parent = layout.add(b4), off_core = layout.add(n);
  const size_t off_offsets = layout.add(b8), off_rec = layout.add(256), off_counts = layout.add(256), off_tmp = layout.add(tmp_bytes);
  const size_t off_labels = layout.add(on_device ? 0 : b4), off_core_out = layout.add(on_device || !core ? 0 : n);
  Scratch scratch(layout, s, who.c_str());
  uint64_t* keys_a = scratch.at<uint64_t>(off_keys_a);
  uint64_t* keys_b = scratch.at<uint64_t>(off_keys_b);
  uint32_t* vals_a = scratch.at<uint32_t>(off_vals_a);
  uint32_t* order = scratch.at<uint32_t>(off_order);
  double* xs = scratch.at<double>(off_xs);
  double* ys = scratch.at<double>(off_ys);
  double* zs = scratch.at<double>(off_zs);
  uint32_t* parent = scratch.at<uint32_t>(off_parent);
  uint8_t* core_sorted = scratch.at<uint8_t>(off_core);
  unsigned long long* offsets = scratch.at<unsigned long long>(off_offsets);
  pstk::ClusterRecord* rec = scratch.at<pstk::ClusterRecord>(off_rec);
  unsigned long long* counts_dev = scratch.at<unsigned long long>(off_counts);  // {core points, labelled points}
  void* tmp = scratch.at<void>(off_tmp);
  uint32_t* labels_dev = on_device ? labels : scratch.at<uint32_t>(off_labels);
  uint8_t* core_dev = !core ? nullptr : on_device ? core : scratch.at<uint8_t>(off_core_out);

  PhaseEvents events;
  events.mark(0, s);
  // ---- index build: AABB of the finite points -> (host: grid) -> keys -> sort -> gather
  if (!pstk::cluster_bounds(pos, rec, s)) throw hip_failure(who + ": bounds launch failed: ");
  pstk::ClusterRecord r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  const uint32_t nf = (uint32_t)r.finite_count;
  if (nf == 0 || min_points > nf) {  // no point can have min_points neighbours: everything is noise
    if (on_device) {
      PST_HIP_CHECK(hipMemsetAsync(labels, 0xFF, n * sizeof(uint32_t), s));
      if (core) PST_HIP_CHECK(hipMemsetAsync(core, 0, n, s));
    } else {
      std::memset(labels, 0xFF, n * sizeof(uint32_t));
      if (core) std::memset(core, 0, n);
    }
    stream_sync(s);
    return PST_OK;
  }
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = pstk::cluster_decode_ordered(r.min_ordered[a]);
    hi[a] = pstk::cluster_decode_ordered(r.max_ordered[a]);
  }
  const pstk::ClusterGrid grid = cluster_grid_over(lo, hi, eps, who);
  const unsigned key_bits = grid.bits[0] + grid.bits[1] + grid.bits[2];
  if (!pstk::cluster_keys(pos, grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure(who + ": key launch failed: ");
  size_t bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::sort_pairs_u64(tmp, bytes, keys_a, keys_b, vals_a, order, n, key_bits + 1, s));
  if (!pstk::nn_gather(pos, order, nf, xs, ys, zs, s)) throw hip_failure(who + ": gather launch failed: ");
  PST_HIP_CHECK(hipMemsetAsync(counts_dev, 0, 2 * sizeof(*counts_dev), s));
  events.mark(1, s);
  // ---- core points
  const unsigned long long* keys = (const unsigned long long*)keys_b;
  if (!pstk::dbscan_count(keys, xs, ys, zs, nf, grid, e2, (uint32_t)min_points, core_sorted, parent, counts_dev, s)) throw hip_failure(who + ": count launch failed: ");
  events.mark(2, s);
  // ---- clusters of the core points
  if (!pstk::dbscan_link(keys, xs, ys, zs, core_sorted, nf, grid, e2, parent, s)) throw hip_failure(who + ": link launch failed: ");
  events.mark(3, s);
  // ---- border points, then the bookkeeping
  uint32_t* root = vals_a;
  const auto [size, min_index] = halves(keys_a);
  if (!pstk::dbscan_border(keys, xs, ys, zs, core_sorted, order, nf, grid, e2, parent, root, size, min_index, s)) throw hip_failure(who + ": border launch failed: ");
  const auto [list_keys, list_roots] = halves(xs);
  const auto [sorted_keys, sorted_roots] = halves(keys_b);
  uint32_t* rank_of_root = halves(ys).first;
  const auto [root_at, flags] = halves(zs);
  if (!pstk::dbscan_flag(root, size, min_index, n, nf, flags, root_at, counts_dev + 1, s)) throw hip_failure(who + ": flag launch failed: ");
  bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, flags, offsets, n + 1, s));
  if (!pstk::cluster_list_kept(flags, offsets, root_at, size, n, list_keys, list_roots, s)) throw hip_failure(who + ": list launch failed: ");
  unsigned long long clusters = 0, counted[2] = {0, 0};
  PST_HIP_CHECK(hipMemcpyAsync(&clusters, offsets + n, sizeof(clusters), hipMemcpyDeviceToHost, s));
  PST_HIP_CHECK(hipMemcpyAsync(counted, counts_dev, sizeof(counted), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  // one STABLE sort on 0xFFFFFFFF - size: descending size, and equal sizes keep the list's order, ascending smallest member
  bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::sort_pairs_u32(tmp, bytes, list_keys, sorted_keys, list_roots, sorted_roots, (size_t)clusters, 32, s));
  unsigned long long* sizes_dev = offsets;  // (the scan's result has been used up)
  if (!pstk::dbscan_labels(sorted_keys, sorted_roots, (uint32_t)clusters, order, root, core_sorted, n, nf, rank_of_root, sizes_dev, labels_dev, core_dev, s))
    throw hip_failure(who + ": label launch failed: ");
  events.mark(4, s);
  const bool sizes_fit = clusters <= sizes_capacity;
  if (sizes && sizes_fit && clusters) PST_HIP_CHECK(hipMemcpyAsync(sizes, sizes_dev, (size_t)clusters * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (!on_device) {
    PST_HIP_CHECK(hipMemcpyAsync(labels, labels_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (core) PST_HIP_CHECK(hipMemcpyAsync(core, core_dev, n, hipMemcpyDeviceToHost, s));
  }
  stream_sync(s);
  events.read();
  counts[0] = clusters;
  counts[1] = counted[0];
  counts[2] = counted[1];
  if (sizes && !sizes_fit)
    throw Error(PST_ERR_RANGE, who + ": " + std::to_string(clusters) + " clusters do not fit the size array of " + std::to_string(sizes_capacity));
  PST_API_END
}

}  // extern "C"
