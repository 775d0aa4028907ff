// pst_segment_statistics / pst_segments_kernel_shape / pst_segments_phase_times: argument checks, the scratch layout, the levels' tables and
// the order of the launches of segments.hip (where the definitions are).
#include <cstring>
#include <memory>
#include <vector>

#include "dense_directory.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

constexpr uint64_t kMaxSegments = 1ull << 28;
constexpr uint32_t kPlanesOfBit[8] = {1, 6, 3, 6, 1, 1, 1, 1};  // count, bounds, centroid, covariance, value min / max / mean / variance

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_SEGMENTS_TIMES=1 (tools/bench_segments.py reads them through pst_segments_phase_times)

uint32_t plane_count(uint32_t stats) {
  uint32_t planes = 0;
  for (int bit = 0; bit < 8; ++bit)
    if (stats & (1u << bit)) planes += kPlanesOfBit[bit];
  return planes;
}

// the planes of the set bits of `stats`, in ascending bit order, S doubles each from `base`
pstk::SegmentPlanes planes_at(double* base, uint32_t stats, size_t S) {
  double* p[8] = {};
  size_t at = 0;
  for (int bit = 0; bit < 8; ++bit)
    if (stats & (1u << bit)) {
      p[bit] = base + at * S;
      at += kPlanesOfBit[bit];
    }
  return pstk::SegmentPlanes{p[0], p[1], p[1] ? p[1] + 3 * S : nullptr, p[2], p[3], p[4], p[5], p[6], p[7]};
}

// One level of the fold: how many elements every segment holds there, in how many groups, and the exclusive sums of both
struct LevelTables {
  Scratch block;
  uint32_t *count = nullptr, *groups = nullptr;
  unsigned long long *element_offset = nullptr, *group_offset = nullptr;
  uint64_t n_elements = 0, n_groups = 0;

  LevelTables(size_t S, hipStream_t s, const char* who) {
    ScratchLayout layout;
    const size_t off_count = layout.add((S + 1) * 4), off_groups = layout.add((S + 1) * 4), off_eo = layout.add((S + 1) * 8), off_go = layout.add((S + 1) * 8);
    block.alloc(layout.total(), s, who);
    count = block.at<uint32_t>(off_count);
    groups = block.at<uint32_t>(off_groups);
    element_offset = block.at<unsigned long long>(off_eo);
    group_offset = block.at<unsigned long long>(off_go);
  }
  // behind the kernel that wrote count and groups: the two sums, their totals read back (synchronises)
  void scan(size_t S, void* tmp, size_t tmp_bytes, hipStream_t s) {
    size_t bytes = tmp_bytes;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, count, element_offset, S + 1, s));
    bytes = tmp_bytes;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, groups, group_offset, S + 1, s));
    unsigned long long totals[2] = {0, 0};
    PST_HIP_CHECK(hipMemcpyAsync(&totals[0], element_offset + S, 8, hipMemcpyDeviceToHost, s));
    PST_HIP_CHECK(hipMemcpyAsync(&totals[1], group_offset + S, 8, hipMemcpyDeviceToHost, s));
    stream_sync(s);
    n_elements = totals[0];
    n_groups = totals[1];
  }
};

// The channels of one pass: what level 0 reads, where the results go; the partials of the levels above live in blocks of run()'s own
struct Pass {
  const double* sum_in[7] = {};
  double* sum_result[7] = {};
  const double* min_in[4] = {};
  double* min_result[4] = {};
  const double* max_in[4] = {};
  double* max_result[4] = {};
  const uint32_t* apex_in = nullptr;
  uint32_t* apex_result = nullptr;
  const double* column[4] = {};
  const double* mean[4] = {};
  bool products = false;

  void run(const std::vector<std::unique_ptr<LevelTables>>& levels, const uint32_t* dir, uint32_t S, hipStream_t s, const char* who) const {
    std::unique_ptr<Scratch> in_block, out_block;
    pstk::SegmentFold f{};
    f.dir = dir;
    f.n_segments = S;
    std::memcpy(f.sum_result, sum_result, sizeof(sum_result));
    std::memcpy(f.min_result, min_result, sizeof(min_result));
    std::memcpy(f.max_result, max_result, sizeof(max_result));
    f.apex_result = apex_result;
    std::memcpy(f.column, column, sizeof(column));
    std::memcpy(f.mean, mean, sizeof(mean));
    std::memcpy(f.sum_in, sum_in, sizeof(sum_in));
    std::memcpy(f.min_in, min_in, sizeof(min_in));
    std::memcpy(f.max_in, max_in, sizeof(max_in));
    f.apex_in = apex_in;
    bool sums[7];  // the sums this pass computes
    for (int c = 0; c < 7; ++c) sums[c] = (products ? (const double*)sum_result[c] : sum_in[c]) != nullptr;
    for (size_t k = 0; k < levels.size(); ++k) {
      const LevelTables& lv = *levels[k];
      const bool more = k + 1 < levels.size();
      f.level = pstk::SegmentLevel{lv.n_groups, lv.group_offset, lv.element_offset, more ? levels[k + 1]->element_offset : nullptr, lv.count};
      std::memset(f.sum_out, 0, sizeof(f.sum_out));
      std::memset(f.min_out, 0, sizeof(f.min_out));
      std::memset(f.max_out, 0, sizeof(f.max_out));
      f.apex_out = nullptr;
      if (more) {  // the partials: one array of the next level's elements per channel
        const size_t e = (size_t)levels[k + 1]->n_elements;
        ScratchLayout layout;
        size_t off_sum[7], off_min[4], off_max[4];
        for (int c = 0; c < 7; ++c) off_sum[c] = layout.add(sums[c] ? e * 8 : 0);
        for (int c = 0; c < 4; ++c) off_min[c] = layout.add(min_in[c] ? e * 8 : 0);
        for (int c = 0; c < 4; ++c) off_max[c] = layout.add(max_in[c] ? e * 8 : 0);
        const size_t off_apex = layout.add(apex_in ? e * 4 : 0);
        out_block.reset(new Scratch(layout, s, who));
        for (int c = 0; c < 7; ++c) f.sum_out[c] = sums[c] ? out_block->at<double>(off_sum[c]) : nullptr;
        for (int c = 0; c < 4; ++c) f.min_out[c] = min_in[c] ? out_block->at<double>(off_min[c]) : nullptr;
        for (int c = 0; c < 4; ++c) f.max_out[c] = max_in[c] ? out_block->at<double>(off_max[c]) : nullptr;
        f.apex_out = apex_in ? out_block->at<uint32_t>(off_apex) : nullptr;
      }
      if (!pstk::segment_fold(f, products && k == 0, s)) throw hip_failure(std::string(who) + ": fold launch failed: ");
      // this level's partials are the next level's elements
      for (int c = 0; c < 7; ++c) f.sum_in[c] = f.sum_out[c];
      for (int c = 0; c < 4; ++c) { f.min_in[c] = f.min_out[c]; f.max_in[c] = f.max_out[c]; }
      f.apex_in = f.apex_out;
      in_block = std::move(out_block);  // (the block read by the launch above is released behind it, in stream order)
    }
  }
};

}  // namespace

extern "C" {

int pst_segments_kernel_shape(uint32_t* points_per_block, uint32_t* group, uint32_t* groups_per_block) {
  if (points_per_block) *points_per_block = pstk::kSegmentsPointsPerBlock;
  if (group) *group = pstk::kSegmentGroup;
  if (groups_per_block) *groups_per_block = pstk::kSegmentsGroupsPerBlock;
  return PST_OK;
}

int pst_segments_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_segment_statistics(const pst_buffer* b, const uint32_t* d_labels, uint32_t n_segments, const double* d_values, const uint8_t* d_mask, uint32_t stats, double* out,
                           uint32_t* apex, uint32_t out_memkind, uint64_t* n_members) {
  PST_API_BEGIN
  const char* who = "pst_segment_statistics";
  not_null(b, "buffer");
  not_null(d_labels, "d_labels");
  not_null(out, "out");
  not_null(n_members, "n_members");
  if (out_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid out memory kind");
  if (stats == 0 || stats > 255)
    throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": stats must be a non-empty set of the bits 1 (count), 2 (bounds), 4 (centroid), 8 (covariance), 16 (value min), "
                                              "32 (value max), 64 (value mean), 128 (value variance)");
  if (n_segments == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": n_segments must not be zero");
  const Member& pm = position_member(*b);
  *n_members = 0;
  ensure_device();
  const size_t n = b->len;
  check_point_count(n, who);
  if (n_segments > kMaxSegments) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 segments");

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  const pstk::SegmentInput in{d_labels, d_values, d_mask};
  static const bool timed = env_nonzero("PST_SEGMENTS_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  const size_t S = n_segments;
  const uint32_t n_planes = plane_count(stats);
  const bool out_on_device = out_memkind == PST_MEM_DEVICE;
  const bool covariance = stats & pstk::SG_COVARIANCE, variance = stats & pstk::SG_VALUE_VARIANCE;
  const bool sum_xyz = stats & (pstk::SG_CENTROID | pstk::SG_COVARIANCE), sum_v = stats & (pstk::SG_VALUE_MEAN | pstk::SG_VALUE_VARIANCE);
  const bool max_v = (stats & pstk::SG_VALUE_MAX) || apex;

  // the planes and the apex (host results only) | the centroid and the mean where the second pass needs what `stats` does not name | the
  // directory over the keys 0 .. S, ix.order = the buffer index of every sorted position | x, y, z, v in sorted order | sort and scan scratch
  size_t scan_bytes = 0;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, S + 1, s));
  ScratchLayout layout;
  const size_t off_stage = layout.add(out_on_device ? 0 : S * 8 * n_planes), off_stage_apex = layout.add(out_on_device || !apex ? 0 : S * 4);
  const size_t off_centroid = layout.add(covariance && !(stats & pstk::SG_CENTROID) ? S * 8 * 3 : 0);
  const size_t off_mean = layout.add(variance && !(stats & pstk::SG_VALUE_MEAN) ? S * 8 : 0);
  DenseDirectory ix;
  ix.carve(layout, plain_keys(pstk::bits_for(S + 1)), S, n, n, s);
  const size_t off_xs = layout.add(n * 8), off_ys = layout.add(n * 8), off_zs = layout.add(n * 8), off_vs = layout.add(d_values ? n * 8 : 0);
  const size_t off_tmp = layout.add(std::max(ix.tmp_bytes(), scan_bytes));
  Scratch scratch(layout, s, who);
  ix.bind(scratch);
  const pstk::SegmentPlanes planes = planes_at(out_on_device ? out : scratch.at<double>(off_stage), stats, S);
  uint32_t* apex_dev = !apex ? nullptr : out_on_device ? apex : scratch.at<uint32_t>(off_stage_apex);
  double* centroid = stats & pstk::SG_CENTROID ? planes.centroid : covariance ? scratch.at<double>(off_centroid) : nullptr;
  double* mean = stats & pstk::SG_VALUE_MEAN ? planes.value_mean : variance ? scratch.at<double>(off_mean) : nullptr;
  uint32_t *order = ix.order, *dir = ix.dir;
  double *xs = scratch.at<double>(off_xs), *ys = scratch.at<double>(off_ys), *zs = scratch.at<double>(off_zs);
  double* vs = d_values ? scratch.at<double>(off_vs) : zs;
  void* tmp = scratch.at<void>(off_tmp);
  const size_t tmp_bytes = layout.total() - off_tmp;

  // ---- keys, sort, directory
  events.mark(0, s);
  ix.build(tmp, s, who, [&](uint32_t* keys) {
    if (!pstk::segment_keys(pos, in, n_segments, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: ");
  });
  events.mark(1, s);
  // ---- gather
  if (n && !pstk::segment_gather(pos, in, order, dir, n_segments, xs, ys, zs, d_values ? vs : nullptr, s)) throw hip_failure(std::string(who) + ": gather launch failed: ");
  events.mark(2, s);
  // ---- the levels' tables: level 0 holds the members; a level follows while a segment has more than one group
  std::vector<std::unique_ptr<LevelTables>> levels;
  levels.emplace_back(new LevelTables(S, s, who));
  if (!pstk::segment_counts(dir, n_segments, planes, apex_dev, levels[0]->count, levels[0]->groups, s)) throw hip_failure(std::string(who) + ": count launch failed: ");
  levels[0]->scan(S, tmp, tmp_bytes, s);
  const uint64_t members = levels[0]->n_elements;
  while (levels.back()->n_groups > 1) {
    std::unique_ptr<LevelTables> next(new LevelTables(S, s, who));
    if (!pstk::segment_next_level(levels.back()->groups, n_segments, next->count, next->groups, s)) throw hip_failure(std::string(who) + ": level launch failed: ");
    next->scan(S, tmp, tmp_bytes, s);
    if (next->n_elements == 0) break;  // every segment has finished
    levels.push_back(std::move(next));
  }
  // ---- the folds: sums and extremes, then the products about the means
  if (members) {
    Pass first;
    const double* cols[4] = {xs, ys, zs, vs};
    for (int c = 0; c < 3; ++c) {
      if (sum_xyz) { first.sum_in[c] = cols[c]; first.sum_result[c] = centroid + c * S; }
      if (stats & pstk::SG_BOUNDS) {
        first.min_in[c] = first.max_in[c] = cols[c];
        first.min_result[c] = planes.min + c * S;
        first.max_result[c] = planes.max + c * S;
      }
    }
    if (sum_v) { first.sum_in[3] = vs; first.sum_result[3] = mean; }
    if (stats & pstk::SG_VALUE_MIN) { first.min_in[3] = vs; first.min_result[3] = planes.value_min; }
    if (max_v) { first.max_in[3] = vs; first.max_result[3] = planes.value_max; }
    if (apex) { first.apex_in = order; first.apex_result = apex_dev; }
    if (sum_xyz || sum_v || (stats & pstk::SG_BOUNDS) || (stats & pstk::SG_VALUE_MIN) || max_v) first.run(levels, dir, n_segments, s, who);
    if (covariance || variance) {
      Pass second;
      second.products = true;
      for (int c = 0; c < 3; ++c)
        if (covariance) { second.column[c] = cols[c]; second.mean[c] = centroid + c * S; }
      for (int c = 0; c < 6; ++c)
        if (covariance) second.sum_result[c] = planes.covariance + c * S;
      if (variance) { second.column[3] = vs; second.mean[3] = mean; second.sum_result[6] = planes.value_variance; }
      second.run(levels, dir, n_segments, s, who);
    }
  }
  events.mark(3, s);
  if (!out_on_device) {
    PST_HIP_CHECK(hipMemcpyAsync(out, scratch.at<double>(off_stage), S * 8 * n_planes, hipMemcpyDeviceToHost, s));
    if (apex) PST_HIP_CHECK(hipMemcpyAsync(apex, apex_dev, S * 4, hipMemcpyDeviceToHost, s));
  }
  stream_sync(s);
  events.read();
  *n_members = members;
  PST_API_END
}

}  // extern "C"
