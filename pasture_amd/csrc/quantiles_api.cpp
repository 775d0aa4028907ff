// pst_rasterize_quantiles / pst_segment_quantiles / pst_quantiles_kernel_shape / pst_quantiles_phase_times: argument checks, the front end
// shared with pst_rasterize and pst_segment_statistics (keys, sort, directory, gather), the scratch layout and the order of the launches of
// quantiles.hip (where the definitions are).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "dense_directory.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

constexpr uint64_t kMaxGroups = 1ull << 28;
constexpr uint32_t kMaxPlanes = 64;

thread_local double t_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};  // PST_QUANTILES_TIMES=1 (tools/bench_quantiles.py reads them through pst_quantiles_phase_times)

// the checks both entry points share, in this order: the plane count, the arrays, every probability, the method, every threshold
pstk::QuantileRequest checked_request(const double* probs, uint32_t n_probs, uint32_t method, const double* thresholds, uint32_t n_thresholds, const std::string& who) {
  const uint64_t planes = (uint64_t)n_probs + n_thresholds;
  if (planes == 0 || planes > kMaxPlanes) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": n_probs + n_thresholds must be 1 .. 64");
  if (n_probs) not_null(probs, "probs");
  if (n_thresholds) not_null(thresholds, "thresholds");
  pstk::QuantileRequest rq{};
  for (uint32_t i = 0; i < n_probs; ++i) {
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": every probability must lie in [0, 1]");
    rq.param[i] = probs[i];
  }
  if (method > pstk::QM_HIGHER) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": method must be 0 (linear), 1 (lower) or 2 (higher)");
  for (uint32_t i = 0; i < n_thresholds; ++i) {
    if (std::isnan(thresholds[i])) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": a threshold must not be NaN");
    rq.param[n_probs + i] = thresholds[i];
  }
  rq.n_probs = n_probs;
  rq.n_thresholds = n_thresholds;
  rq.method = method;
  return rq;
}

// The body of both calls.  fill_keys(keys_a) launches the key kernel; key_bits: the keys' width; G groups.  Returns the number of members.
template <class FillKeys>
uint64_t order_statistics(const pstk::Positions& pos, const pstk::RasterInput& in, size_t G, unsigned key_bits, const pstk::QuantileRequest& rq, double* out,
                          uint32_t out_memkind, hipStream_t s, const char* who, FillKeys fill_keys) {
  static const bool timed = env_nonzero("PST_QUANTILES_TIMES");
  static const bool general = env_nonzero("PST_QUANTILES_GENERAL");  // A/B: every group takes the path of the large ones
  const uint32_t cap = general ? 0 : pstk::kQuantilesCap;
  PhaseEvents<4> events(timed, t_phase_ms);
  const size_t n = pos.n;
  const uint32_t n_planes = 1 + rq.n_probs + rq.n_thresholds;
  const bool out_on_device = out_memkind == PST_MEM_DEVICE;
  const size_t heavy_capacity = pstk::quantile_heavy_capacity(n, G, cap);

  // the planes (host results only) | the directory, ix.order = the buffer index of every sorted position | the values in sorted order | the
  // large groups, their sizes, the sizes' exclusive sum, their number | sort and scan scratch
  size_t scan_bytes = 0;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, heavy_capacity + 1, s));
  ScratchLayout layout;
  const size_t off_stage = layout.add(out_on_device ? 0 : G * 8 * n_planes);
  DenseDirectory ix;
  ix.carve(layout, plain_keys(key_bits), G, n, n, s);
  const size_t off_values = layout.add(n * 8);
  const size_t off_heavy = layout.add((heavy_capacity + 1) * 4), off_heavy_size = layout.add((heavy_capacity + 1) * 4), off_heavy_offset = layout.add((heavy_capacity + 1) * 8);
  const size_t off_heavy_count = layout.add(256), off_tmp = layout.add(std::max(ix.tmp_bytes(), scan_bytes));
  Scratch scratch(layout, s, who);
  ix.bind(scratch);
  double* planes = out_on_device ? out : scratch.at<double>(off_stage);
  uint32_t *keys_b = ix.keys_b, *order = ix.order, *dir = ix.dir;
  uint32_t *heavy_list = scratch.at<uint32_t>(off_heavy), *heavy_size = scratch.at<uint32_t>(off_heavy_size), *heavy_count = scratch.at<uint32_t>(off_heavy_count);
  unsigned long long* heavy_offset = scratch.at<unsigned long long>(off_heavy_offset);
  double* values = scratch.at<double>(off_values);
  void* tmp = scratch.at<void>(off_tmp);

  // ---- keys, sort, directory
  events.mark(0, s);
  PST_HIP_CHECK(hipMemsetAsync(heavy_count, 0, sizeof(*heavy_count), s));
  ix.build(tmp, s, who, fill_keys);
  events.mark(1, s);
  // ---- gather
  if (n && !pstk::raster_gather(pos, in, order, dir, (uint32_t)G, values, s)) throw hip_failure(std::string(who) + ": gather launch failed: ");
  events.mark(2, s);
  // ---- COUNT, the empty groups, the list of the large ones; the small groups
  if (!pstk::quantile_groups(dir, (uint32_t)G, cap, rq, planes, heavy_list, heavy_size, heavy_count, s)) throw hip_failure(std::string(who) + ": group launch failed: ");
  if (!pstk::quantile_small_groups(values, keys_b, dir, (uint32_t)n, (uint32_t)G, cap, rq, planes, s)) throw hip_failure(std::string(who) + ": window launch failed: ");
  events.mark(3, s);
  // ---- the large groups
  uint32_t members = 0, heavy = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&members, dir + G, sizeof(members), hipMemcpyDeviceToHost, s));
  PST_HIP_CHECK(hipMemcpyAsync(&heavy, heavy_count, sizeof(heavy), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  if (heavy) {
    unsigned long long listed = 0;  // (heavy <= heavy_capacity: that many groups of more than cap members there can be)
    PST_HIP_CHECK(hipMemsetAsync(heavy_size + heavy, 0, 4, s));
    size_t bytes = scan_bytes;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, heavy_size, heavy_offset, (size_t)heavy + 1, s));
    PST_HIP_CHECK(hipMemcpyAsync(&listed, heavy_offset + heavy, sizeof(listed), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    const size_t L = (size_t)listed;  // <= members
    const unsigned owner_bits = pstk::bits_for(heavy);
    size_t sort64_bytes = 0, sort32_bytes = 0;
    PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort64_bytes, nullptr, nullptr, nullptr, nullptr, L, 64, s));
    PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort32_bytes, nullptr, nullptr, nullptr, nullptr, L, owner_bits, s));
    // value keys a | b | slots a | slots by value | owner | owner keys a | b | the slots by (owner, value) | sort scratch
    ScratchLayout hl;
    const size_t off_ka = hl.add(L * 8), off_kb = hl.add(L * 8), off_sa = hl.add(L * 4), off_sb = hl.add(L * 4), off_owner = hl.add(L * 4);
    const size_t off_oa = hl.add(L * 4), off_ob = hl.add(L * 4), off_ranked = hl.add(L * 4), off_htmp = hl.add(std::max(sort64_bytes, sort32_bytes));
    Scratch hs(hl, s, who);
    uint64_t *ka = hs.at<uint64_t>(off_ka), *kb = hs.at<uint64_t>(off_kb);
    uint32_t *sa = hs.at<uint32_t>(off_sa), *sb = hs.at<uint32_t>(off_sb), *owner = hs.at<uint32_t>(off_owner);
    uint32_t *oa = hs.at<uint32_t>(off_oa), *ob = hs.at<uint32_t>(off_ob), *ranked = hs.at<uint32_t>(off_ranked);
    if (!pstk::quantile_heavy_compact(values, dir, heavy_list, heavy_offset, heavy, (uint32_t)L, (unsigned long long*)ka, sa, owner, s))
      throw hip_failure(std::string(who) + ": compaction launch failed: ");
    bytes = sort64_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u64(hs.at<void>(off_htmp), bytes, ka, kb, sa, sb, L, 64, s));
    if (!pstk::quantile_owner_gather(owner, sb, (uint32_t)L, oa, s)) throw hip_failure(std::string(who) + ": owner launch failed: ");
    bytes = sort32_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u32(hs.at<void>(off_htmp), bytes, oa, ob, sb, ranked, L, owner_bits, s));
    if (!pstk::quantile_heavy_select(values, dir, (uint32_t)G, heavy_list, heavy_offset, heavy, ranked, rq, planes, s))
      throw hip_failure(std::string(who) + ": selection launch failed: ");
  }
  events.mark(4, s);
  if (!out_on_device) PST_HIP_CHECK(hipMemcpyAsync(out, planes, G * 8 * n_planes, hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  return members;
}

}  // namespace

extern "C" {

int pst_quantiles_kernel_shape(uint32_t* points_per_block, uint32_t* cap, uint32_t* window) {
  if (points_per_block) *points_per_block = pstk::kQuantilesPointsPerBlock;
  if (cap) *cap = pstk::kQuantilesCap;
  if (window) *window = pstk::kQuantilesWindow;
  return PST_OK;
}

int pst_quantiles_phase_times(double ms[4]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_rasterize_quantiles(const pst_buffer* b, const double* d_values, const uint8_t* d_mask, double cell_size, const double origin[2], const uint32_t dim[2],
                            const double* probs, uint32_t n_probs, uint32_t method, const double* thresholds, uint32_t n_thresholds, double* out, uint32_t out_memkind,
                            double origin_out[2], uint32_t dim_out[2], uint64_t* n_members) {
  PST_API_BEGIN
  const char* who = "pst_rasterize_quantiles";
  not_null(b, "buffer");
  not_null(out, "out");
  not_null(n_members, "n_members");
  if (out_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid out memory kind");
  if (!std::isfinite(cell_size) || !(cell_size > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": cell_size must be finite and positive");
  const pstk::QuantileRequest rq = checked_request(probs, n_probs, method, thresholds, n_thresholds, who);
  if ((origin == nullptr) != (dim == nullptr)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": origin and dim must be given together or not at all");
  const bool given = origin != nullptr;
  pstk::PmfGrid grid{};
  if (given) {
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1])) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": origin must be finite");
    if (dim[0] == 0 || dim[1] == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": dim must not hold a zero");
    if ((uint64_t)dim[0] * dim[1] > kMaxGroups) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": the raster would have more than 2^28 cells: use a larger cell_size");
    grid = pstk::PmfGrid{origin[0], origin[1], cell_size, dim[0], dim[1]};
  }
  const Member& pm = position_member(*b);
  *n_members = 0;
  const auto report = [&](const pstk::PmfGrid& g) {
    if (origin_out) { origin_out[0] = g.x0; origin_out[1] = g.y0; }
    if (dim_out) { dim_out[0] = g.cols; dim_out[1] = g.rows; }
  };
  report(grid);  // (zeros for the automatic grid until there is one)
  const size_t n = b->len;
  if (n == 0 && !given) return PST_OK;  // no points, no grid: nothing to write
  ensure_device();
  check_point_count(n, who);

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  if (!given) {
    const pstk::HagBounds r = finite_bounds_2d(pos, nullptr, s, who);  // of the finite points, whatever the mask says
    if (r.count == 0) return PST_OK;  // nothing but non-finite points: no grid, `out` untouched
    grid = pmf_grid_over(r.min_x, r.min_y, r.max_x, r.max_y, cell_size, who);
  }
  const size_t cells = (size_t)grid.cols * grid.rows;
  const unsigned cell_bits = pstk::bits_for(cells);
  const uint32_t nonmember_key = 1u << cell_bits;  // at most 2^28
  const pstk::RasterInput in{d_values, d_mask};
  const uint64_t members = order_statistics(pos, in, cells, cell_bits + 1, rq, out, out_memkind, s, who, [&](uint32_t* keys) {
    if (!pstk::raster_keys(pos, in, grid, nonmember_key, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: ");
  });
  report(grid);
  *n_members = members;
  PST_API_END
}

int pst_segment_quantiles(const pst_buffer* b, const uint32_t* d_labels, uint32_t n_segments, const double* d_values, const uint8_t* d_mask, const double* probs,
                          uint32_t n_probs, uint32_t method, const double* thresholds, uint32_t n_thresholds, double* out, uint32_t out_memkind, uint64_t* n_members) {
  PST_API_BEGIN
  const char* who = "pst_segment_quantiles";
  not_null(b, "buffer");
  not_null(d_labels, "d_labels");
  not_null(out, "out");
  not_null(n_members, "n_members");
  if (out_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid out memory kind");
  const pstk::QuantileRequest rq = checked_request(probs, n_probs, method, thresholds, n_thresholds, who);
  if (n_segments == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": n_segments must not be zero");
  const Member& pm = position_member(*b);
  *n_members = 0;
  ensure_device();
  const size_t n = b->len;
  check_point_count(n, who);
  if (n_segments > kMaxGroups) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 segments");

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  const pstk::SegmentInput sin{d_labels, d_values, d_mask};
  const pstk::RasterInput in{d_values, d_mask};  // (the gather: the value column or z of the members the keys chose)
  const uint64_t members = order_statistics(pos, in, n_segments, pstk::bits_for((uint64_t)n_segments + 1), rq, out, out_memkind, s, who, [&](uint32_t* keys) {
    if (!pstk::segment_keys(pos, sin, n_segments, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: ");
  });
  *n_members = members;
  PST_API_END
}

}  // extern "C"
