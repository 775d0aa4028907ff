// pst_euclidean_clusters / pst_cluster_mask_device / pst_cluster_kernel_shape: argument checks, the scratch layout and the order of the
// launches of clusters.hip (where the definitions and the argument for the grid's margin are; the grid is cluster_grid.hpp's, the index build
// cluster_index.hpp's, the numbering and the copies to the outputs cluster_numbering.hpp's).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "cluster_numbering.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_CLUSTER_TIMES=1 (tools/bench_clusters.py reads them through pst_cluster_phase_times)

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
  const Member& pm = position_member(*b);
  ensure_device();
  check_point_count(b->len, who);
  *n_clusters = 0;
  *n_clustered = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points, no clusters, no labels to write

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
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
  ScratchLayout layout;
  ClusterIndex ix;
  ix.carve(layout, n);
  const size_t off_parent = layout.add(ix.b4), off_offsets = layout.add(2 * ix.b4);
  const size_t off_rec = layout.add(256), off_tmp = layout.add(tmp_bytes), off_labels = layout.add(labels_on_device ? 0 : ix.b4);
  Scratch scratch(layout, s, who.c_str());
  ix.bind(scratch);
  uint32_t* parent = scratch.at<uint32_t>(off_parent);
  unsigned long long* offsets = scratch.at<unsigned long long>(off_offsets);
  pstk::ClusterRecord* rec = scratch.at<pstk::ClusterRecord>(off_rec);
  void* tmp = scratch.at<void>(off_tmp);
  uint32_t* labels_dev = labels_on_device ? labels : scratch.at<uint32_t>(off_labels);
  uint32_t* const order = ix.order;

  static const bool timed = env_nonzero("PST_CLUSTER_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  events.mark(0, s);
  // ---- index build: AABB of the finite points -> (host: grid) -> keys -> sort (the gather is the traversal launcher's)
  const FiniteBounds bounds = finite_bounds(pos, rec, s, who);
  const uint32_t nf = (uint32_t)bounds.count;
  if (nf == 0) {  // nothing but non-finite points: every label is "none"
    fill_result(labels, 0xFF, n * sizeof(uint32_t), labels_on_device, s);
    stream_sync(s);
    return PST_OK;
  }
  const pstk::ClusterGrid grid = cluster_grid_over(bounds, tolerance, who);
  ix.build(pos, grid, nf, tmp, tmp_bytes, s, who, false);
  // ---- traversal + union
  if (!pstk::cluster_components(pos, grid, t2, ix.sorted_keys(), order, nf, ix.xs, ix.ys, ix.zs, parent, s, events.event(1)))
    throw hip_failure("cluster traversal launch failed: ");
  events.mark(2, s);
  // ---- bookkeeping
  const auto [root, size] = ix.halves(ix.xs);
  const auto [min_index, root_at] = ix.halves(ix.ys);
  uint32_t* flags = ix.halves(ix.zs).first;
  const auto [list_keys, list_roots] = ix.halves(ix.keys_a);
  const auto [sorted_keys, sorted_roots] = ix.halves(ix.keys_b);
  uint32_t* rank_of_root = ix.vals_a;
  if (!pstk::cluster_flatten(parent, order, nf, root, size, min_index, s)) throw hip_failure(who + ": flatten launch failed: ");
  // (the two counters: the record's finite_count, which nobody reads again, and its `clustered`, zero since the bounds pass)
  const NumberingArrays arrays{root, size, min_index, flags, root_at, list_keys, list_roots, sorted_keys, sorted_roots, rank_of_root, offsets, &rec->finite_count, tmp, tmp_bytes};
  const Numbered numbered = number_kept(arrays, n, nf, min_size, max_size, s, who);
  if (!pstk::cluster_labels(order, root, rank_of_root, n, nf, labels_dev, s)) throw hip_failure(who + ": label launch failed: ");
  events.mark(3, s);
  finish_numbered(numbered, NumberedOutputs{labels_on_device, labels, labels_dev, nullptr, nullptr, sizes, sizes_capacity, n_clusters, nullptr, n_clustered}, n, events, s, who,
                  "clusters");
  PST_API_END
}

}  // extern "C"
