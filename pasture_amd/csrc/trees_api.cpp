// pst_tree_tops_device / pst_segment_trees_device / pst_trees_kernel_shape / pst_trees_phase_times / pst_trees_work: argument checks, the
// grids (hag_grid.hpp, trees_window.hpp), the scratch layouts and the order of the launches of trees.hip (where the definitions and the
// exactness arguments are).
#include <cmath>
#include <cstring>
#include <limits>

#include "dense_directory.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};  // PST_TREES_TIMES=1 (tools/bench_trees.py reads them through pst_trees_phase_times)
thread_local uint64_t t_work[3] = {0, 0, 0};               // candidates, survivors of the near pass, candidates the far pass tested (PST_TREES_WORK=1)

constexpr double kInf = std::numeric_limits<double>::infinity();

void check_edge(double cell_edge, const char* who) {
  if (!(cell_edge >= 0.0) || std::isinf(cell_edge)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": cell_edge must be finite and not negative (0: automatic)");
}

// the member byte of a call and the record of its bounds, read back (one synchronisation)
pstk::TreesBounds members_of(const pstk::TreesInput& in, const uint8_t* also, double floor, uint8_t* member, hipStream_t s, const char* who) {
  ScratchLayout layout;
  const size_t off_partials = layout.add(pstk::trees_bounds_partials_bytes(in.pos.n)), off_rec = layout.add(sizeof(pstk::TreesBounds));
  Scratch block(layout, s, who);
  pstk::TreesBounds* rec = block.at<pstk::TreesBounds>(off_rec);
  if (!pstk::trees_members(in, also, floor, member, block.at<void>(off_partials), rec, s)) throw hip_failure(std::string(who) + ": member launch failed: ");
  pstk::TreesBounds r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  return r;
}

pstk::HagGrid grid_over(const pstk::TreesBounds& b, double edge, const char* who) {
  pstk::HagGrid grid{};
  if (!pstk::hag_make_grid(b.min_x, b.min_y, b.max_x, b.max_y, edge, &grid)) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": the extent of the indexed points overflows f64");
  return grid;
}

// The dense directory over `count` entries (entry e = point subset ? subset[e] : e; the m members first in cell order) and, in the same
// block of scratch, the members' x, y, h and buffer index in sorted order.
struct TreeIndex : DenseDirectory {
  size_t off_m[4] = {};
  uint32_t* index = nullptr;
  double *xs = nullptr, *ys = nullptr, *hs = nullptr;

  void carve(ScratchLayout& layout, const pstk::HagGrid& grid, size_t count, size_t m, hipStream_t s) {
    DenseDirectory::carve(layout, packed_keys(grid), (size_t)grid.dim[0] * grid.dim[1], count, count, s);
    const size_t bytes[4] = {m * 4, m * 8, m * 8, m * 8};
    for (int i = 0; i < 4; ++i) off_m[i] = layout.add(bytes[i]);
  }
  void bind(Scratch& scratch) {
    DenseDirectory::bind(scratch);
    index = scratch.at<uint32_t>(off_m[0]);
    xs = scratch.at<double>(off_m[1]); ys = scratch.at<double>(off_m[2]); hs = scratch.at<double>(off_m[3]);
  }
  // (the heads kernel looks at the m members alone)
  void build(const pstk::TreesInput& in, const uint32_t* subset, const uint8_t* member, uint32_t m, const pstk::HagGrid& grid, void* tmp, hipStream_t s, const char* who) {
    DenseDirectory::build(m, tmp, s, who,
                          [&](uint32_t* keys) { if (!pstk::trees_keys(in.pos, subset, member, count, grid, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: "); },
                          [&] { if (!pstk::trees_gather(in, subset, order, m, xs, ys, hs, index, s)) throw hip_failure(std::string(who) + ": gather launch failed: "); });
  }
};

// The numbering: the points a byte flags, by descending height, ties by ascending buffer index.  flags -> exclusive sum -> the ascending
// list with the order-reversing image of every height -> the stable 64-bit pair sort.  `list` (device, in `block`) holds the nt buffer
// indices in tree order afterwards.  Synchronises once, to size the sort.
struct Numbering {
  Scratch counted, block;
  uint32_t* list = nullptr;
  uint32_t nt = 0;

  void run(const pstk::TreesInput& in, const uint8_t* bytes, hipStream_t s, const char* who) {
    const size_t n = in.pos.n;
    size_t scan_bytes = 0;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
    ScratchLayout first;
    const size_t off_flags = first.add((n + 1) * 4), off_offsets = first.add((n + 1) * 8), off_scan = first.add(scan_bytes);
    counted.alloc(first.total(), s, who);
    uint32_t* flags = counted.at<uint32_t>(off_flags);
    unsigned long long* offsets = counted.at<unsigned long long>(off_offsets);
    if (!pstk::trees_flags(bytes, n, flags, s)) throw hip_failure(std::string(who) + ": flag launch failed: ");
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(counted.at<void>(off_scan), scan_bytes, flags, offsets, n + 1, s));
    unsigned long long total = 0;
    PST_HIP_CHECK(hipMemcpyAsync(&total, offsets + n, sizeof(total), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    nt = (uint32_t)total;
    if (nt == 0) return;
    size_t sort_bytes = 0;
    PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, nt, 64, s));
    ScratchLayout second;
    const size_t off_ka = second.add((size_t)nt * 8), off_kb = second.add((size_t)nt * 8), off_va = second.add((size_t)nt * 4), off_vb = second.add((size_t)nt * 4);
    const size_t off_tmp = second.add(sort_bytes);
    block.alloc(second.total(), s, who);
    uint64_t *ka = block.at<uint64_t>(off_ka), *kb = block.at<uint64_t>(off_kb);
    uint32_t* va = block.at<uint32_t>(off_va);
    list = block.at<uint32_t>(off_vb);
    if (!pstk::trees_list(in, flags, offsets, n, (unsigned long long*)ka, va, s)) throw hip_failure(std::string(who) + ": list launch failed: ");
    PST_HIP_CHECK(pstk::sort_pairs_u64(block.at<void>(off_tmp), sort_bytes, ka, kb, va, list, nt, 64, s));
  }
};

pstk::TreesInput input_of(const pst_buffer& b, const double* d_heights, const uint8_t* d_mask) {
  return pstk::TreesInput{positions_of(b, position_member(b)), d_heights, d_mask};
}

}  // namespace

extern "C" {

int pst_trees_kernel_shape(uint32_t* points_per_block, uint32_t* survivors_per_block, uint32_t* queries_per_block, uint32_t* bounds_points_per_block) {
  if (points_per_block) *points_per_block = pstk::kTreesPointsPerBlock;
  if (survivors_per_block) *survivors_per_block = pstk::kTreesSurvivorsPerBlock;
  if (queries_per_block) *queries_per_block = pstk::kTreesQueriesPerBlock;
  if (bounds_points_per_block) *bounds_points_per_block = pstk::kTreesBoundsPointsPerBlock;
  return PST_OK;
}

int pst_trees_phase_times(double ms[4]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_trees_work(uint64_t out[3]) {
  PST_API_BEGIN
  not_null(out, "out");
  std::memcpy(out, t_work, sizeof(t_work));
  PST_API_END
}

int pst_tree_tops_device(const pst_buffer* b, const double* d_heights, const uint8_t* d_mask, double min_height, const double window[4], double cell_edge,
                         uint8_t* d_top_mask, uint32_t* d_top_indices, size_t capacity, uint64_t* n_candidates, uint64_t* n_tops, double grid_min_and_edge[3],
                         uint32_t grid_dim[2]) {
  PST_API_BEGIN
  const char* who = "pst_tree_tops_device";
  not_null(b, "buffer");
  not_null(window, "window");
  if (!std::isfinite(min_height)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": min_height must be finite");
  const pstk::TreeWindow w{window[0], window[1], window[2], window[3]};
  if (!std::isfinite(w.a) || !std::isfinite(w.b) || !std::isfinite(w.r_min) || !(w.r_min >= 0.0) || !(w.r_max >= w.r_min))
    throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": window = {a, b, r_min, r_max} needs finite a, b and 0 <= r_min <= r_max with r_min finite (r_max may be +inf)");
  check_edge(cell_edge, who);
  const pstk::TreesInput in = input_of(*b, d_heights, d_mask);
  if (n_candidates) *n_candidates = 0;
  if (n_tops) *n_tops = 0;
  if (grid_min_and_edge) grid_min_and_edge[0] = grid_min_and_edge[1] = grid_min_and_edge[2] = 0.0;
  if (grid_dim) grid_dim[0] = grid_dim[1] = 0;
  t_work[0] = t_work[1] = t_work[2] = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no point: nothing to write
  not_null(d_top_mask, "d_top_mask");
  ensure_device();
  check_point_count(n, who);

  hipStream_t s = current_stream();
  static const bool timed = env_nonzero("PST_TREES_TIMES");
  static const bool counted = env_nonzero("PST_TREES_WORK");
  PhaseEvents<4> events(timed, t_phase_ms);
  events.mark(0, s);
  // ---- the candidates and their index
  Scratch member_block;
  uint8_t* member = member_block.alloc<uint8_t>(n, s, who);
  const pstk::TreesBounds bounds = members_of(in, nullptr, min_height, member, s, who);
  const uint32_t nc = (uint32_t)bounds.count;
  PST_HIP_CHECK(hipMemsetAsync(d_top_mask, 0, n, s));
  if (nc == 0) {  // no candidate: no top, a zero grid
    for (int i = 1; i <= 4; ++i) events.mark(i, s);
    stream_sync(s);
    events.read();
    return PST_OK;
  }
  // The automatic edge: HALF the radius of a window at half the largest |h|.  With an edge of a whole radius every box would lie inside the
  // 3 x 3 cells and the near pass, one lane per candidate, would walk whole windows; at half of it the near pass sees the neighbours within
  // 0.5 - 1 radius, which decide nearly every candidate of a canopy, and what is left -- the tops, mostly -- gets a wave each.  Not below
  // the edge that puts about one candidate into the 3 x 3 cells (hag_auto_edge, k = 1 asks for two): the directory is 4 bytes per cell.  It
  // affects speed only.
  double edge = cell_edge;
  if (!(edge > 0.0)) {
    const double sparse = pstk::hag_auto_edge(nc, bounds.max_x - bounds.min_x, bounds.max_y - bounds.min_y, 1) * 0.5;
    const double half_window = 0.5 * pstk::trees_window_radius(w, 0.5 * bounds.max_abs_h);
    edge = std::isfinite(half_window) && half_window > sparse ? half_window : sparse;
  }
  const pstk::HagGrid grid = grid_over(bounds, edge, who);
  ScratchLayout layout;
  TreeIndex ix;
  ix.carve(layout, grid, n, nc, s);
  size_t scan_bytes = 0;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, (size_t)nc + 1, s));
  const size_t off_flags = layout.add(((size_t)nc + 1) * 4), off_offsets = layout.add(((size_t)nc + 1) * 8), off_survivors = layout.add((size_t)nc * 4);
  const size_t off_tmp = layout.add(std::max(ix.tmp_bytes(), scan_bytes)), off_work = layout.add(256);
  Scratch scratch(layout, s, who);
  ix.bind(scratch);
  uint32_t *flags = scratch.at<uint32_t>(off_flags), *survivors = scratch.at<uint32_t>(off_survivors);
  unsigned long long *offsets = scratch.at<unsigned long long>(off_offsets), *work = scratch.at<unsigned long long>(off_work);
  void* tmp = scratch.at<void>(off_tmp);
  ix.build(in, nullptr, member, nc, grid, tmp, s, who);
  events.mark(1, s);
  // ---- the filter: the near pass, the survivors' list, the far pass
  PST_HIP_CHECK(hipMemsetAsync(work, 0, sizeof(*work), s));
  if (!pstk::trees_filter_near(w, grid, ix.dir, ix.xs, ix.ys, ix.hs, ix.index, nc, d_top_mask, flags, s)) throw hip_failure(std::string(who) + ": near launch failed: ");
  size_t bytes = scan_bytes;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, flags, offsets, (size_t)nc + 1, s));
  if (!pstk::sample_compact(nullptr, flags, offsets, nc, survivors, s)) throw hip_failure(std::string(who) + ": compaction launch failed: ");
  unsigned long long n_survivors = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&n_survivors, offsets + nc, sizeof(n_survivors), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  if (!pstk::trees_filter_far(w, grid, ix.dir, ix.xs, ix.ys, ix.hs, ix.index, survivors, (uint32_t)n_survivors, d_top_mask, counted ? work : nullptr, s))
    throw hip_failure(std::string(who) + ": far launch failed: ");
  unsigned long long tested = 0;
  if (counted) PST_HIP_CHECK(hipMemcpyAsync(&tested, work, sizeof(tested), hipMemcpyDeviceToHost, s));
  events.mark(2, s);
  // ---- the numbering
  Numbering numbering;
  numbering.run(in, d_top_mask, s, who);
  const uint32_t nt = numbering.nt;
  const bool fits = nt <= capacity;
  if (d_top_indices && fits && nt) PST_HIP_CHECK(hipMemcpyAsync(d_top_indices, numbering.list, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
  events.mark(3, s);
  events.mark(4, s);
  stream_sync(s);
  events.read();
  t_work[0] = nc; t_work[1] = n_survivors; t_work[2] = tested;
  if (n_candidates) *n_candidates = nc;
  if (n_tops) *n_tops = nt;
  if (grid_min_and_edge) { grid_min_and_edge[0] = grid.min[0]; grid_min_and_edge[1] = grid.min[1]; grid_min_and_edge[2] = grid.edge; }
  if (grid_dim) { grid_dim[0] = grid.dim[0]; grid_dim[1] = grid.dim[1]; }
  if (d_top_indices && !fits)
    throw Error(PST_ERR_RANGE, std::string(who) + ": " + std::to_string(nt) + " tops do not fit the index array of " + std::to_string(capacity));
  PST_API_END
}

int pst_segment_trees_device(const pst_buffer* b, const double* d_heights, const uint8_t* d_mask, const uint8_t* d_top_mask, double min_height, double max_crown_factor,
                             double exclusion, double cell_edge, uint32_t* d_tree_id, uint32_t* d_tree_counts, size_t counts_capacity, uint64_t* n_trees,
                             uint64_t* n_labelled) {
  PST_API_BEGIN
  const char* who = "pst_segment_trees_device";
  not_null(b, "buffer");
  if (!std::isfinite(min_height)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": min_height must be finite");
  if (!(max_crown_factor >= 0.0) || std::isinf(max_crown_factor)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_crown_factor must be finite and not negative");
  if (!(exclusion >= 0.0 && exclusion <= 1.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": exclusion must lie in [0, 1]");
  check_edge(cell_edge, who);
  const pstk::TreesInput in = input_of(*b, d_heights, d_mask);
  if (n_trees) *n_trees = 0;
  if (n_labelled) *n_labelled = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no point: nothing to write
  not_null(d_top_mask, "d_top_mask");
  not_null(d_tree_id, "d_tree_id");
  ensure_device();
  check_point_count(n, who);

  hipStream_t s = current_stream();
  static const bool timed = env_nonzero("PST_TREES_TIMES");
  PhaseEvents<4> events(timed, t_phase_ms);
  for (int i = 0; i <= 2; ++i) events.mark(i, s);
  // ---- the trees: the flagged valid points, whatever their height, numbered
  Scratch member_block;
  uint8_t* member = member_block.alloc<uint8_t>(n, s, who);
  const pstk::TreesBounds bounds = members_of(in, d_top_mask, -kInf, member, s, who);
  Numbering numbering;
  if (bounds.count) numbering.run(in, member, s, who);
  const uint32_t nt = numbering.nt;
  events.mark(3, s);
  if (nt == 0) {  // no tree: no label
    PST_HIP_CHECK(hipMemsetAsync(d_tree_id, 0xFF, n * 4, s));
    events.mark(4, s);
    stream_sync(s);
    events.read();
    return PST_OK;
  }
  // ---- the index of the tops (entry t = tree t) and the queries in cell order
  const double edge = cell_edge > 0.0 ? cell_edge : pstk::hag_auto_edge(nt, bounds.max_x - bounds.min_x, bounds.max_y - bounds.min_y, 1);
  const pstk::HagGrid grid = grid_over(bounds, edge, who);
  // The search may stop at rc_max = half_factor * max |H|: rc_t = half_factor * H_t, and a product with a fixed non-negative factor and a
  // square of an absolute value are both monotone under rounding, so rc_t * rc_t <= rc_max * rc_max for every tree -- a top farther away
  // than that fails its own test d2 <= rc_t * rc_t anyway (trees.hip).  max |H|, not max H: a top below zero has a positive rc * rc.
  const double half_factor = 0.5 * max_crown_factor;
  const double rc_max = half_factor * bounds.max_abs_h;
  const double m2 = rc_max * rc_max;
  ScratchLayout layout;
  TreeIndex ix;
  ix.carve(layout, grid, nt, nt, s);
  size_t sort_q = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_q, nullptr, nullptr, nullptr, nullptr, n, ix.keys.bits, s));
  const size_t off_qa = layout.add(n * 4), off_qb = layout.add(n * 4), off_qv = layout.add(n * 4), off_qorder = layout.add(n * 4);
  const size_t off_tmp = layout.add(std::max(ix.tmp_bytes(), sort_q)), off_counts = layout.add((size_t)nt * 4), off_labelled = layout.add(256);
  Scratch scratch(layout, s, who);
  ix.bind(scratch);
  uint32_t *qa = scratch.at<uint32_t>(off_qa), *qb = scratch.at<uint32_t>(off_qb), *qv = scratch.at<uint32_t>(off_qv), *qorder = scratch.at<uint32_t>(off_qorder);
  uint32_t* counts = scratch.at<uint32_t>(off_counts);
  unsigned long long* labelled = scratch.at<unsigned long long>(off_labelled);
  void* tmp = scratch.at<void>(off_tmp);
  PST_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)nt * 4, s));
  PST_HIP_CHECK(hipMemsetAsync(labelled, 0, sizeof(*labelled), s));
  ix.build(in, numbering.list, nullptr, nt, grid, tmp, s, who);  // (ix.order[s] = the tree number of sorted top s)
  if (!pstk::trees_query_keys(in, min_height, grid, qa, qv, s)) throw hip_failure(std::string(who) + ": query key launch failed: ");
  size_t bytes = sort_q;
  PST_HIP_CHECK(pstk::sort_pairs_u32(tmp, bytes, qa, qb, qv, qorder, n, ix.keys.bits, s));
  // ---- the search
  if (!pstk::trees_crown_search(in, (uint32_t)n, grid, m2, half_factor, exclusion, qb, qorder, ix.dir, ix.xs, ix.ys, ix.hs, ix.index, ix.order, d_tree_id, counts, labelled, s))
    throw hip_failure(std::string(who) + ": search launch failed: ");
  const bool fits = nt <= counts_capacity;
  if (d_tree_counts && fits) PST_HIP_CHECK(hipMemcpyAsync(d_tree_counts, counts, (size_t)nt * 4, hipMemcpyDeviceToDevice, s));
  events.mark(4, s);
  unsigned long long total = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&total, labelled, sizeof(total), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  if (n_trees) *n_trees = nt;
  if (n_labelled) *n_labelled = total;
  if (d_tree_counts && !fits)
    throw Error(PST_ERR_RANGE, std::string(who) + ": " + std::to_string(nt) + " trees do not fit the count array of " + std::to_string(counts_capacity));
  PST_API_END
}

}  // extern "C"
