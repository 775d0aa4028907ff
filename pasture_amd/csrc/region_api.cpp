// pst_region_growing_from_knn / pst_region_growing / pst_region_kernel_shape / pst_region_phase_times: argument checks, the scratch layout
// and the order of the launches of region.hip (where the pipeline is laid out; the definition is in include/pasture_amd.h).  The full call
// puts the kNN search (knn_checks.hpp) and the feature kernel (features.hip: e3 and the surface variation) in front of it; the numbering
// and the copies to the outputs behind it are cluster_numbering.hpp's.
#include <cmath>
#include <cstring>

#include "cluster_numbering.hpp"
#include "knn_checks.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_REGION_TIMES=1 (tools/bench_region.py reads them through pst_region_phase_times)

struct RegionArgs {
  double min_abs_cos, curvature_threshold, max_distance;
  uint64_t min_size, max_size;
  uint32_t* labels;
  uint8_t* smooth;
  uint32_t memkind;
  uint64_t* sizes;
  size_t sizes_capacity;
  uint64_t* counts;
};

// what both entries ask of their parameters, before a device is looked for
void check_region_args(const RegionArgs& a, const std::string& who) {
  not_null(a.labels, "labels");
  not_null(a.counts, "counts");
  if (a.memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid labels memory kind");
  if (!(a.min_abs_cos >= 0.0 && a.min_abs_cos <= 1.0)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": min_abs_cos must lie in [0, 1]");
  if (std::isnan(a.curvature_threshold)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": curvature_threshold must not be NaN");
  if (std::isnan(a.max_distance) || a.max_distance < 0.0) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": max_distance must not be negative or NaN (+inf: no limit)");
  if (a.min_size == 0) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": min_size must be at least 1");
  if (a.max_size < a.min_size) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": max_size must not be below min_size");
}

// The regions' own scratch, carved behind whatever the caller put into the layout first.  Everything is 4 bytes per point unless noted:
//   state (1), parent, root, size, min_index, flags (n + 1), root_at, offsets (8 (n + 1): the scan; then the sizes), the regions' list
//   (keys | roots) unsorted and sorted, rank of every root, counts, sort / scan scratch, labels and smooth mask (host outputs only)
struct RegionWork {
  size_t n = 0, b4 = 0, tmp_bytes = 0;
  size_t off_state = 0, off_parent = 0, off_root = 0, off_size = 0, off_min = 0, off_flags = 0, off_root_at = 0, off_offsets = 0, off_list = 0, off_sorted = 0,
         off_rank = 0, off_counts = 0, off_tmp = 0, off_labels = 0, off_smooth = 0;
  void carve(ScratchLayout& layout, size_t points, const RegionArgs& a, hipStream_t s) {
    n = points;
    b4 = n * sizeof(uint32_t);
    size_t sort_bytes = 0, scan_bytes = 0;
    PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 32, s));
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
    tmp_bytes = std::max(sort_bytes, scan_bytes);
    const bool on_device = a.memkind == PST_MEM_DEVICE;
    off_state = layout.add(n);
    off_parent = layout.add(b4);
    off_root = layout.add(b4);
    off_size = layout.add(b4);
    off_min = layout.add(b4);
    off_flags = layout.add(b4 + sizeof(uint32_t));
    off_root_at = layout.add(b4);
    off_offsets = layout.add(2 * b4 + sizeof(uint64_t));
    off_list = layout.add(2 * b4);
    off_sorted = layout.add(2 * b4);
    off_rank = layout.add(b4);
    off_counts = layout.add(256);
    off_tmp = layout.add(tmp_bytes);
    off_labels = layout.add(on_device ? 0 : b4);
    off_smooth = layout.add(on_device || !a.smooth ? 0 : n);
  }
};

// classify + link, attach + numbering (number_kept, the label kernel, finish_numbered): marks events 1 .. 3 (the caller marked 0 in front of whatever it ran itself)
void run_regions(const pstk::Positions& pos, uint32_t k, const uint32_t* d_knn, const double* d_normals, const double* d_curvature, const RegionArgs& a, RegionWork& w,
                 Scratch& scratch, PhaseEvents<3>& events, hipStream_t s, const std::string& who) {
  const uint32_t n = (uint32_t)w.n;
  const bool on_device = a.memkind == PST_MEM_DEVICE;
  uint8_t* state = scratch.at<uint8_t>(w.off_state);
  uint32_t *parent = scratch.at<uint32_t>(w.off_parent), *root = scratch.at<uint32_t>(w.off_root), *size = scratch.at<uint32_t>(w.off_size),
           *min_index = scratch.at<uint32_t>(w.off_min), *flags = scratch.at<uint32_t>(w.off_flags), *root_at = scratch.at<uint32_t>(w.off_root_at),
           *rank_of_root = scratch.at<uint32_t>(w.off_rank);
  uint32_t *list_keys = scratch.at<uint32_t>(w.off_list), *list_roots = list_keys + n, *sorted_keys = scratch.at<uint32_t>(w.off_sorted), *sorted_roots = sorted_keys + n;
  unsigned long long* offsets = scratch.at<unsigned long long>(w.off_offsets);
  unsigned long long* counts_dev = scratch.at<unsigned long long>(w.off_counts);  // {smooth points, labelled points}
  void* tmp = scratch.at<void>(w.off_tmp);
  uint32_t* labels_dev = on_device ? a.labels : scratch.at<uint32_t>(w.off_labels);
  uint8_t* smooth_dev = !a.smooth ? nullptr : on_device ? a.smooth : scratch.at<uint8_t>(w.off_smooth);

  events.mark(1, s);
  // ---- smooth points, then their regions
  PST_HIP_CHECK(hipMemsetAsync(counts_dev, 0, 2 * sizeof(*counts_dev), s));
  if (!pstk::region_classify(d_normals, d_curvature, a.curvature_threshold, n, state, parent, counts_dev, s)) throw hip_failure(who + ": classify launch failed: ");
  if (!pstk::region_link(pos, k, d_knn, d_normals, state, a.min_abs_cos, a.max_distance, parent, s)) throw hip_failure(who + ": link launch failed: ");
  events.mark(2, s);
  // ---- rim points, then the bookkeeping
  if (!pstk::region_attach(pos, k, d_knn, d_normals, state, a.min_abs_cos, a.max_distance, parent, root, size, min_index, s)) throw hip_failure(who + ": attach launch failed: ");
  const NumberingArrays arrays{root, size, min_index, flags, root_at, list_keys, list_roots, sorted_keys, sorted_roots, rank_of_root, offsets, counts_dev, tmp, w.tmp_bytes};
  const Numbered numbered = number_kept(arrays, w.n, n, a.min_size, a.max_size, s, who);
  if (!pstk::region_labels(root, rank_of_root, state, n, labels_dev, smooth_dev, s)) throw hip_failure(who + ": label launch failed: ");
  events.mark(3, s);
  finish_numbered(numbered, NumberedOutputs{on_device, a.labels, labels_dev, a.smooth, smooth_dev, a.sizes, a.sizes_capacity, a.counts, a.counts + 1, a.counts + 2}, w.n, events,
                  s, who, "regions");
}

bool timed() {
  static const bool on = env_nonzero("PST_REGION_TIMES");
  return on;
}

}  // namespace

extern "C" {

int pst_region_kernel_shape(size_t k, uint32_t* points_per_block, uint32_t* threads) {
  PST_API_BEGIN
  if (k < 1 || k > 64) throw Error(PST_ERR_INVALID_ARGUMENT, "pst_region_kernel_shape: k must be between 1 and 64");
  if (points_per_block) *points_per_block = pstk::region_points_per_block((uint32_t)k);
  if (threads) *threads = pstk::kRegionThreads;
  PST_API_END
}

int pst_region_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_region_growing_from_knn(const pst_buffer* b, size_t k, const uint32_t* d_knn, const double* d_normals, const double* d_curvature, double min_abs_cos,
                                double curvature_threshold, double max_distance, uint64_t min_size, uint64_t max_size, uint32_t* labels, uint8_t* smooth, uint32_t memkind,
                                uint64_t* sizes, size_t sizes_capacity, uint64_t counts[3]) {
  PST_API_BEGIN
  const std::string who = "pst_region_growing_from_knn";
  not_null(b, "buffer");
  not_null(d_knn, "d_knn");
  not_null(d_normals, "d_normals");
  const RegionArgs a{min_abs_cos, curvature_threshold, max_distance, min_size, max_size, labels, smooth, memkind, sizes, sizes_capacity, counts};
  check_region_args(a, who);
  if (k < 1 || k > 64) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": k must be between 1 and 64");
  const Member& pm = position_member(*b);
  counts[0] = counts[1] = counts[2] = 0;
  if (b->len == 0) return PST_OK;  // no points: no regions, no label and no mask byte to write
  ensure_device();
  check_point_count(b->len, who);

  hipStream_t s = current_stream();
  ScratchLayout layout;
  RegionWork w;
  w.carve(layout, b->len, a, s);
  Scratch scratch(layout, s, who.c_str());
  PhaseEvents<3> events(timed(), t_phase_ms);
  events.mark(0, s);
  run_regions(positions_of(*b, pm), (uint32_t)k, d_knn, d_normals, d_curvature, a, w, scratch, events, s, who);
  PST_API_END
}

int pst_region_growing(const pst_buffer* b, size_t k, double min_abs_cos, double curvature_threshold, double max_distance, uint64_t min_size, uint64_t max_size,
                       uint32_t* labels, uint8_t* smooth, uint32_t memkind, uint64_t* sizes, size_t sizes_capacity, uint64_t counts[3], double* d_normals,
                       double* d_curvature, uint32_t* d_knn) {
  PST_API_BEGIN
  const std::string who = "pst_region_growing";
  not_null(b, "buffer");
  const RegionArgs a{min_abs_cos, curvature_threshold, max_distance, min_size, max_size, labels, smooth, memkind, sizes, sizes_capacity, counts};
  check_region_args(a, who);
  const Member& pm = knn_checked_arguments(*b, k, who.c_str());
  ensure_device();
  counts[0] = counts[1] = counts[2] = 0;
  if (b->len == 0) return PST_OK;  // no points: nothing to search
  knn_checked_length(*b, 3, who.c_str());

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  const size_t n = pos.n;
  ScratchLayout layout;
  const size_t off_normals = layout.add(d_normals ? 0 : n * 3 * sizeof(double)), off_curvature = layout.add(d_curvature ? 0 : n * sizeof(double)),
               off_knn = layout.add(d_knn ? 0 : n * k * sizeof(uint32_t));
  RegionWork w;
  w.carve(layout, n, a, s);
  Scratch scratch(layout, s, who.c_str());
  if (!d_normals) d_normals = scratch.at<double>(off_normals);
  if (!d_curvature) d_curvature = scratch.at<double>(off_curvature);
  if (!d_knn) d_knn = scratch.at<uint32_t>(off_knn);
  PhaseEvents<3> events(timed(), t_phase_ms);
  events.mark(0, s);
  // ---- the lists, then e3 and l3 / S from them
  knn_lists(pos, k, d_knn, s, who.c_str());
  if (!pstk::geometric_features(pos, (uint32_t)k, d_knn, max_distance, PST_FEATURE_SURFACE_VARIATION, d_curvature, d_normals, nullptr, s))
    throw hip_failure(who + ": feature launch failed: ");
  run_regions(pos, (uint32_t)k, d_knn, d_normals, d_curvature, a, w, scratch, events, s, who);
  PST_API_END
}

}  // extern "C"
