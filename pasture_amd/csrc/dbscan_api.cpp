// pst_dbscan / pst_dbscan_kernel_shape / pst_dbscan_phase_times: argument checks, the scratch layout and the order of the launches of
// dbscan.hip (where the pipeline is laid out; the definitions are in include/pasture_amd.h, the argument for the grid's margin at the head
// of clusters.hip; the grid is cluster_grid.hpp's, the index build cluster_index.hpp's, the numbering and the copies to the outputs
// cluster_numbering.hpp's).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "cluster_numbering.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};  // PST_DBSCAN_TIMES=1 (tools/bench_dbscan.py reads them through pst_dbscan_phase_times)

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
  const Member& pm = position_member(*b);
  ensure_device();
  check_point_count(b->len, who);
  counts[0] = counts[1] = counts[2] = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points: no clusters, no label and no core byte to write

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
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
  ScratchLayout layout;
  ClusterIndex ix;
  ix.carve(layout, n);
  const size_t off_parent = layout.add(ix.b4), off_core = layout.add(n);
  const size_t off_offsets = layout.add(2 * ix.b4), off_rec = layout.add(256), off_counts = layout.add(256), off_tmp = layout.add(tmp_bytes);
  const size_t off_labels = layout.add(on_device ? 0 : ix.b4), off_core_out = layout.add(on_device || !core ? 0 : n);
  Scratch scratch(layout, s, who.c_str());
  ix.bind(scratch);
  uint32_t* const order = ix.order;
  double *const xs = ix.xs, *const ys = ix.ys, *const zs = ix.zs;
  uint32_t* parent = scratch.at<uint32_t>(off_parent);
  uint8_t* core_sorted = scratch.at<uint8_t>(off_core);
  unsigned long long* offsets = scratch.at<unsigned long long>(off_offsets);
  pstk::ClusterRecord* rec = scratch.at<pstk::ClusterRecord>(off_rec);
  unsigned long long* counts_dev = scratch.at<unsigned long long>(off_counts);  // {core points, labelled points}
  void* tmp = scratch.at<void>(off_tmp);
  uint32_t* labels_dev = on_device ? labels : scratch.at<uint32_t>(off_labels);
  uint8_t* core_dev = !core ? nullptr : on_device ? core : scratch.at<uint8_t>(off_core_out);

  static const bool timed = env_nonzero("PST_DBSCAN_TIMES");
  PhaseEvents<4> events(timed, t_phase_ms);
  events.mark(0, s);
  // ---- index build: AABB of the finite points -> (host: grid) -> keys -> sort -> gather
  const FiniteBounds bounds = finite_bounds(pos, rec, s, who);
  const uint32_t nf = (uint32_t)bounds.count;
  if (nf == 0 || min_points > nf) {  // no point can have min_points neighbours: everything is noise
    fill_result(labels, 0xFF, n * sizeof(uint32_t), on_device, s);
    if (core) fill_result(core, 0, n, on_device, s);
    stream_sync(s);
    return PST_OK;
  }
  const pstk::ClusterGrid grid = cluster_grid_over(bounds, eps, who);
  ix.build(pos, grid, nf, tmp, tmp_bytes, s, who, true);
  PST_HIP_CHECK(hipMemsetAsync(counts_dev, 0, 2 * sizeof(*counts_dev), s));
  events.mark(1, s);
  // ---- core points
  const unsigned long long* keys = ix.sorted_keys();
  if (!pstk::dbscan_count(keys, xs, ys, zs, nf, grid, e2, (uint32_t)min_points, core_sorted, parent, counts_dev, s)) throw hip_failure(who + ": count launch failed: ");
  events.mark(2, s);
  // ---- clusters of the core points
  if (!pstk::dbscan_link(keys, xs, ys, zs, core_sorted, nf, grid, e2, parent, s)) throw hip_failure(who + ": link launch failed: ");
  events.mark(3, s);
  // ---- border points, then the bookkeeping
  uint32_t* root = ix.vals_a;
  const auto [size, min_index] = ix.halves(ix.keys_a);
  if (!pstk::dbscan_border(keys, xs, ys, zs, core_sorted, order, nf, grid, e2, parent, root, size, min_index, s)) throw hip_failure(who + ": border launch failed: ");
  const auto [list_keys, list_roots] = ix.halves(xs);
  const auto [sorted_keys, sorted_roots] = ix.halves(ix.keys_b);
  uint32_t* rank_of_root = ix.halves(ys).first;
  const auto [root_at, flags] = ix.halves(zs);
  const NumberingArrays arrays{root, size, min_index, flags, root_at, list_keys, list_roots, sorted_keys, sorted_roots, rank_of_root, offsets, counts_dev, tmp, tmp_bytes};
  const Numbered numbered = number_kept(arrays, n, nf, 1, UINT64_MAX, s, who);  // (there is no size filter)
  if (!pstk::dbscan_labels(order, root, rank_of_root, core_sorted, n, nf, labels_dev, core_dev, s)) throw hip_failure(who + ": label launch failed: ");
  events.mark(4, s);
  finish_numbered(numbered, NumberedOutputs{on_device, labels, labels_dev, core, core_dev, sizes, sizes_capacity, counts, counts + 1, counts + 2}, n, events, s, who, "clusters");
  PST_API_END
}

}  // extern "C"
