// pst_euclidean_clusters / pst_cluster_mask_device / pst_cluster_kernel_shape: argument checks, the grid, the scratch layout and the order of the
// launches of clusters.hip (where the definitions and the argument for the grid's margin are).
#include <cmath>
#include <cstring>
#include <utility>

#include "device_sort.hpp"
#include "runtime.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};

// PST_CLUSTER_TIMES=1: stream events around the three phases of every call (tools/bench_clusters.py reads them through pst_cluster_phase_times)
struct PhaseEvents {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool on;
  PhaseEvents() {
    static const bool wanted = env_nonzero("PST_CLUSTER_TIMES");
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
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      if (on) PST_HIP_CHECK(hipEventElapsedTime(&ms, e[i], e[i + 1]));
      t_phase_ms[i] = ms;
    }
  }
};

}  // namespace

extern "C" {

int pst_cluster_kernel_shape(uint32_t* points_per_block, uint32_t* tile_points) {
  if (points_per_block) *points_per_block = pstk::kClusterPointsPerBlock;
  if (tile_points) *tile_points = pstk::kClusterTilePoints;
  return PST_OK;
}

int pst_cluster_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_cluster_mask_device(const uint32_t* d_labels, uint64_t n, uint32_t first_cluster, uint32_t cluster_count, uint8_t* d_mask) {
  PST_API_BEGIN
  if (n == 0) return PST_OK;
  not_null(d_labels, "d_labels");
  not_null(d_mask, "d_mask");
  ensure_device();
  if (!pstk::cluster_mask(d_labels, n, first_cluster, cluster_count, d_mask, current_stream())) throw hip_failure("cluster mask launch failed: ");
  PST_API_END
}

int pst_euclidean_clusters(const pst_buffer* b, double tolerance, uint64_t min_size, uint64_t max_size, uint32_t* labels, uint32_t labels_memkind, uint64_t* sizes,
                           size_t sizes_capacity, uint64_t* n_clusters, uint64_t* n_clustered) {
  PST_API_BEGIN
  const std::string who = "pst_euclidean_clusters";
  not_null(b, "buffer");
  not_null(labels, "labels");
  not_null(n_clusters, "n_clusters");
  not_null(n_clustered, "n_clustered");
  if (labels_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid labels memory kind");
  const double t2 = tolerance * tolerance;
  if (!std::isfinite(tolerance) || !(tolerance > 0.0) || !std::isnormal(t2))
    throw Error(PST_ERR_INVALID_ARGUMENT, who + ": tolerance must be finite and positive, and its square a normal number");
  if (min_size == 0 || min_size > max_size) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": min_size must be at least 1 and not above max_size");
  const Member* pm = position_vec3f64(*b);
  if (!pm) throw Error(PST_ERR_MISSING_ATTRIBUTE, "Attribute not found in PointLayout of buffer");
  ensure_device();
  if (b->len >= 0xFFFFFFF0ull) throw Error(PST_ERR_UNSUPPORTED, who + ": more than 2^32 - 17 points per call");
  *n_clusters = 0;
  *n_clustered = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points, no clusters, no labels to write

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, *pm);
  const bool labels_on_device = labels_memkind == PST_MEM_DEVICE;

  // One block of scratch.  The sort's input pair and the sorted positions are dead once the traversal has run; the bookkeeping lives in them:
  //   keys_a (8n)      unsorted keys            -> the kept clusters' list (keys | roots), unsorted
  //   keys_b (8n)      sorted keys              -> the same list, sorted (behind the traversal)
  //   vals_a (4n)      unsorted indices         -> rank of every root
  //   order  (4n)      buffer index of sorted position s, to the end
  //   xs, ys, zs (8n)  sorted positions         -> root | size, smallest member | root of the flagged point, flags (n + 1)
  //   parent (4n), offsets (8(n + 1): the scan; then the kept sizes), record, sort / scan scratch, labels (host labels only)
  size_t sort64_bytes = 0, sort32_bytes = 0, scan_bytes = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort64_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort32_bytes, nullptr, nullptr, nullptr, nullptr, n, 32, s));
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
  const size_t tmp_bytes = std::max(sort64_bytes, std::max(sort32_bytes, scan_bytes));
  const size_t b4 = up256((n + 1) * 4), b8 = 2 * b4;  // an 8-byte array's room is exactly two 4-byte arrays' (the halves are used as such)
  const auto halves = [b4](void* p) { return std::pair<uint32_t*, uint32_t*>{(uint32_t*)p, (uint32_t*)((uint8_t*)p + b4)}; };
  ScratchLayout layout;
  const size_t off_keys_a = layout.add(b8), off_keys_b = layout.add(b8), off_vals_a = layout.add(b4), off_order = layout.add(b4);
  const size_t off_xs = layout.add(b8), off_ys = layout.add(b8), off_zs = layout.add(b8), off_parent = layout.add(b4), off_offsets = layout.add(b8);
  const size_t off_rec = layout.add(256), off_tmp = layout.add(tmp_bytes), off_labels = layout.add(labels_on_device ? 0 : b4);
  Scratch scratch(layout, s, who.c_str());
  uint64_t* keys_a = scratch.at<uint64_t>(off_keys_a);
  uint64_t* keys_b = scratch.at<uint64_t>(off_keys_b);
  uint32_t* vals_a = scratch.at<uint32_t>(off_vals_a);
  uint32_t* order = scratch.at<uint32_t>(off_order);
  double* xs = scratch.at<double>(off_xs);
  double* ys = scratch.at<double>(off_ys);
  double* zs = scratch.at<double>(off_zs);
  uint32_t* parent = scratch.at<uint32_t>(off_parent);
  unsigned long long* offsets = scratch.at<unsigned long long>(off_offsets);
  pstk::ClusterRecord* rec = scratch.at<pstk::ClusterRecord>(off_rec);
  void* tmp = scratch.at<void>(off_tmp);
  uint32_t* labels_dev = labels_on_device ? labels : scratch.at<uint32_t>(off_labels);

  PhaseEvents events;
  events.mark(0, s);
  // ---- index build: AABB of the finite points -> (host: grid) -> keys -> sort -> gather
  if (!pstk::cluster_bounds(pos, rec, s)) throw hip_failure("cluster bounds launch failed: ");
  pstk::ClusterRecord r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  const uint32_t nf = (uint32_t)r.finite_count;
  if (nf == 0) {  // nothing but non-finite points: every label is "none"
    if (labels_on_device) PST_HIP_CHECK(hipMemsetAsync(labels, 0xFF, n * sizeof(uint32_t), s));
    else std::memset(labels, 0xFF, n * sizeof(uint32_t));
    stream_sync(s);
    return PST_OK;
  }
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = pstk::cluster_decode_ordered(r.min_ordered[a]);
    hi[a] = pstk::cluster_decode_ordered(r.max_ordered[a]);
  }
  const pstk::ClusterGrid grid = cluster_grid_over(lo, hi, tolerance, who);
  const unsigned key_bits = grid.bits[0] + grid.bits[1] + grid.bits[2];
  if (!pstk::cluster_keys(pos, grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure("cluster key launch failed: ");
  size_t bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::sort_pairs_u64(tmp, bytes, keys_a, keys_b, vals_a, order, n, key_bits + 1, s));
  // ---- traversal + union
  if (!pstk::cluster_components(pos, grid, t2, (const unsigned long long*)keys_b, order, nf, xs, ys, zs, parent, s, events.on ? events.e[1] : nullptr))
    throw hip_failure("cluster traversal launch failed: ");
  events.mark(2, s);
  // ---- bookkeeping
  const auto [root, size] = halves(xs);
  const auto [min_index, root_at] = halves(ys);
  uint32_t* flags = halves(zs).first;
  const auto [list_keys, list_roots] = halves(keys_a);
  const auto [sorted_keys, sorted_roots] = halves(keys_b);
  uint32_t* rank_of_root = vals_a;
  if (!pstk::cluster_flag_kept(parent, order, n, nf, min_size, max_size, root, size, min_index, flags, root_at, rec, s)) throw hip_failure("cluster flatten launch failed: ");
  bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, flags, offsets, n + 1, s));
  if (!pstk::cluster_list_kept(flags, offsets, root_at, size, n, list_keys, list_roots, s)) throw hip_failure("cluster list launch failed: ");
  unsigned long long kept = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&kept, offsets + n, sizeof(kept), hipMemcpyDeviceToHost, s));
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  // one STABLE sort on 0xFFFFFFFF - size: descending size, and equal sizes keep the list's order, ascending smallest member
  bytes = tmp_bytes;
  PST_HIP_CHECK(pstk::sort_pairs_u32(tmp, bytes, list_keys, sorted_keys, list_roots, sorted_roots, (size_t)kept, 32, s));
  unsigned long long* sizes_dev = offsets;  // (the scan's result has been used up)
  if (!pstk::cluster_labels(sorted_keys, sorted_roots, (uint32_t)kept, order, root, n, nf, rank_of_root, sizes_dev, labels_dev, s))
    throw hip_failure("cluster label launch failed: ");
  events.mark(3, s);
  const bool sizes_fit = kept <= sizes_capacity;
  if (sizes && sizes_fit && kept) PST_HIP_CHECK(hipMemcpyAsync(sizes, sizes_dev, (size_t)kept * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (!labels_on_device) PST_HIP_CHECK(hipMemcpyAsync(labels, labels_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  *n_clusters = kept;
  *n_clustered = r.clustered;
  if (sizes && !sizes_fit)
    throw Error(PST_ERR_RANGE, who + ": " + std::to_string(kept) + " clusters do not fit the size array of " + std::to_string(sizes_capacity));
  PST_API_END
}

}  // extern "C"
