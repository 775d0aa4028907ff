// pst_pmf_schedule / pst_pmf_grid / pst_pmf_ground_mask / pst_grid_morphology_device / pst_finite_mask_device / pst_buffer_set_u8_where_device /
// pst_pmf_kernel_shape / pst_pmf_phase_times: argument checks, the window schedule, the raster's geometry, the scratch layout and the order of the launches of
// pmf.hip (where the definitions and the argument for splitting a large half-width into passes are).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

constexpr uint64_t kMaxCells = 1ull << 28;

// the seven parameters of the header, as the entry points receive them
struct Params { double cell_size, max_window_size, slope, initial_distance, max_distance; int exponential; uint32_t base; };

struct Schedule {
  uint32_t n = 0;
  uint32_t half_width[pstk::kPmfMaxWindows];
  double threshold[pstk::kPmfMaxWindows];
};

// the parameter checks and the schedule of the header's definition, on the host
Schedule make_schedule(const Params& p, const std::string& who) {
  const auto finite_not_negative = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (!std::isfinite(p.cell_size) || !(p.cell_size > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": cell_size must be finite and positive");
  if (!finite_not_negative(p.max_window_size) || !finite_not_negative(p.slope) || !finite_not_negative(p.initial_distance) || !finite_not_negative(p.max_distance))
    throw Error(PST_ERR_INVALID_ARGUMENT, who + ": max_window_size, slope, initial_distance and max_distance must be finite and not negative");
  if (p.base < (p.exponential ? 2u : 1u)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": base must be at least 2 for an exponential schedule and at least 1 for a linear one");
  Schedule s;
  uint64_t h = p.exponential ? 1 : p.base, w_before = 0;
  for (uint32_t k = 0;; ++k) {
    if (k == pstk::kPmfMaxWindows || h > 0x3FFFFFFFull)
      throw Error(PST_ERR_INVALID_ARGUMENT, who + ": the schedule has more than 32 windows before it reaches max_window_size: use a larger cell, base or a smaller window");
    const uint64_t w = 2 * h + 1;
    double th = p.initial_distance;
    if (k > 0) {
      th = p.slope * (double)(w - w_before) * p.cell_size + p.initial_distance;  // Zhang et al. 2003, eq. 7
      th = p.max_distance < th ? p.max_distance : th;
    }
    s.half_width[k] = (uint32_t)h;
    s.threshold[k] = th;
    s.n = k + 1;
    if ((double)w * p.cell_size >= p.max_window_size) break;
    w_before = w;
    h = p.exponential ? h * p.base : h + p.base;
  }
  return s;
}

// the raster over the finite points' AABB: dim = cell of the largest coordinate + 1, by the expression pmf.hip evaluates per point
pstk::PmfGrid make_grid(const FiniteBounds& b, double cell, const std::string& who) { return pmf_grid_over(b.min[0], b.min[1], b.max[0], b.max[1], cell, who); }

// the AABB of the finite points, read back through a small block of its own: the size of the call's scratch depends on it
FiniteBounds finite_bounds(const pstk::Positions& pos, hipStream_t s, const std::string& who) {
  Scratch block;
  return pst::finite_bounds(pos, block.alloc<pstk::ClusterRecord>(256, s, who.c_str()), s, who);
}

// A run of passes.  erode / dilate by h = the passes along the columns, then those along the rows; along an axis of d cells a half-width
// beyond d - 1 reaches nothing more, and what is left runs in pieces of at most kPmfMaxHalfWidth.  The passes go from `cur` into whichever of
// the two buffers `cur` is not (never in place).
struct Passes {
  uint32_t cols, rows;
  double* bufs[2];
  hipStream_t stream;
  const void* cur;
  bool cur_is_keys;

  static uint32_t pieces(uint32_t h) { return h == 0 ? 1 : (h + pstk::kPmfMaxHalfWidth - 1) / pstk::kPmfMaxHalfWidth; }
  uint32_t reach(uint32_t h, int axis) const { return std::min(h, (axis == 0 ? cols : rows) - 1); }
  uint32_t count(uint32_t h) const { return pieces(reach(h, 0)) + pieces(reach(h, 1)); }
  // L, fold, th: folded by the last pass
  void run(uint32_t h, bool dilate, double* L = nullptr, int fold = 0, double th = 0.0) {
    for (int axis = 0; axis < 2; ++axis) {
      uint32_t left = reach(h, axis);
      for (uint32_t i = pieces(left); i > 0; --i) {
        const uint32_t piece = std::min(left, pstk::kPmfMaxHalfWidth);
        left -= piece;
        const bool last = axis == 1 && i == 1;
        double* out = cur == bufs[0] ? bufs[1] : bufs[0];
        if (!pstk::pmf_morphology_pass(cur, cur_is_keys, out, cols, rows, piece, dilate, axis, last ? L : nullptr, last ? fold : 0, th, stream))
          throw hip_failure("grid morphology launch failed: ");
        cur = out;
        cur_is_keys = false;
      }
    }
  }
};

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_PMF_TIMES=1 (tools/bench_ground.py reads them through pst_pmf_phase_times)

}  // namespace

extern "C" {

int pst_pmf_kernel_shape(uint32_t* points_per_block, uint32_t* tile_cols, uint32_t* tile_rows, uint32_t* max_half_width) {
  if (points_per_block) *points_per_block = pstk::kPmfPointsPerBlock;
  if (tile_cols) *tile_cols = pstk::kPmfTileCols;
  if (tile_rows) *tile_rows = pstk::kPmfTileRows;
  if (max_half_width) *max_half_width = pstk::kPmfMaxHalfWidth;
  return PST_OK;
}

int pst_pmf_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_pmf_schedule(double cell_size, double max_window_size, double slope, double initial_distance, double max_distance, int exponential, uint32_t base, uint32_t half_widths[32],
                     double thresholds[32], uint32_t* n_windows) {
  PST_API_BEGIN
  not_null(n_windows, "n_windows");
  const Schedule s = make_schedule(Params{cell_size, max_window_size, slope, initial_distance, max_distance, exponential, base}, "pst_pmf_schedule");
  for (uint32_t k = 0; k < s.n; ++k) {
    if (half_widths) half_widths[k] = s.half_width[k];
    if (thresholds) thresholds[k] = s.threshold[k];
  }
  *n_windows = s.n;
  PST_API_END
}

int pst_pmf_grid(const pst_buffer* b, double cell_size, double origin[2], uint32_t dim[2], uint64_t* n_finite) {
  PST_API_BEGIN
  const std::string who = "pst_pmf_grid";
  not_null(b, "buffer");
  not_null(origin, "origin");
  not_null(dim, "dim");
  not_null(n_finite, "n_finite");
  if (!std::isfinite(cell_size) || !(cell_size > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": cell_size must be finite and positive");
  const Member& pm = position_member(*b);
  origin[0] = origin[1] = 0.0;
  dim[0] = dim[1] = 0;
  *n_finite = 0;
  if (b->len == 0) return PST_OK;
  ensure_device();
  check_point_count(b->len, who);
  const FiniteBounds r = finite_bounds(positions_of(*b, pm), current_stream(), who);
  if (r.count == 0) return PST_OK;
  const pstk::PmfGrid g = make_grid(r, cell_size, who);
  origin[0] = g.x0;
  origin[1] = g.y0;
  dim[0] = g.cols;
  dim[1] = g.rows;
  *n_finite = r.count;
  PST_API_END
}

int pst_pmf_ground_mask(const pst_buffer* b, double cell_size, double max_window_size, double slope, double initial_distance, double max_distance, int exponential, uint32_t base,
                        uint8_t* mask, uint32_t mask_memkind, double* surfaces, uint32_t surfaces_memkind, uint64_t* n_ground) {
  PST_API_BEGIN
  const std::string who = "pst_pmf_ground_mask";
  not_null(b, "buffer");
  not_null(mask, "mask");
  not_null(n_ground, "n_ground");
  if (mask_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid mask memory kind");
  if (surfaces_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid surfaces memory kind");
  const Schedule sched = make_schedule(Params{cell_size, max_window_size, slope, initial_distance, max_distance, exponential, base}, who);
  const Member& pm = position_member(*b);
  *n_ground = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points: no raster, no ground, no byte to write
  ensure_device();
  check_point_count(n, who);

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  const bool mask_on_device = mask_memkind == PST_MEM_DEVICE;
  static const bool timed = env_nonzero("PST_PMF_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  events.mark(0, s);
  const FiniteBounds r = finite_bounds(pos, s, who);
  if (r.count == 0) {  // nothing but non-finite points: no raster, no ground
    fill_result(mask, 0, n, mask_on_device, s);
    stream_sync(s);
    return PST_OK;
  }
  const pstk::PmfGrid grid = make_grid(r, cell_size, who);
  const size_t cells = (size_t)grid.cols * grid.rows;

  // One block of scratch, 32 bytes per cell: the min-z raster (keys; decoded in place at the end when the surfaces are asked for) | the two
  // rasters the passes alternate between | L | the ground count | the mask (host masks only)
  ScratchLayout layout;
  const size_t off_keys = layout.add(cells * 8), off_a = layout.add(cells * 8), off_b = layout.add(cells * 8), off_l = layout.add(cells * 8);
  const size_t off_count = layout.add(256), off_mask = layout.add(mask_on_device ? 0 : n);
  Scratch scratch(layout, s, who.c_str());
  unsigned long long* keys = scratch.at<unsigned long long>(off_keys);
  double* L = scratch.at<double>(off_l);
  unsigned long long* count = scratch.at<unsigned long long>(off_count);
  uint8_t* mask_dev = mask_on_device ? mask : scratch.at<uint8_t>(off_mask);

  // ---- raster
  PST_HIP_CHECK(hipMemsetAsync(keys, 0xFF, cells * 8, s));  // all ones: empty
  PST_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(*count), s));
  if (!pstk::pmf_raster(pos, grid, keys, s)) throw hip_failure(who + ": raster launch failed: ");
  events.mark(1, s);
  // ---- the openings: the first erosion pass decodes the keys, the last dilation pass of every window folds D + th into L
  Passes passes{grid.cols, grid.rows, {scratch.at<double>(off_a), scratch.at<double>(off_b)}, s, keys, true};
  for (uint32_t k = 0; k < sched.n; ++k) {
    passes.run(sched.half_width[k], false);
    passes.run(sched.half_width[k], true, L, k == 0 ? 1 : 2, sched.threshold[k]);
  }
  events.mark(2, s);
  // ---- classification
  if (!pstk::pmf_classify(pos, grid, L, mask_dev, count, s)) throw hip_failure(who + ": classification launch failed: ");
  events.mark(3, s);
  unsigned long long ground = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&ground, count, sizeof(ground), hipMemcpyDeviceToHost, s));
  if (!mask_on_device) PST_HIP_CHECK(hipMemcpyAsync(mask, mask_dev, n, hipMemcpyDeviceToHost, s));
  if (surfaces) {  // [3][rows][cols]: Z_0, the last opened surface, L
    if (!pstk::pmf_decode_keys(keys, cells, s)) throw hip_failure(who + ": decode launch failed: ");
    const hipMemcpyKind kind = surfaces_memkind == PST_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const void* from[3] = {keys, passes.cur, L};
    for (int i = 0; i < 3; ++i) PST_HIP_CHECK(hipMemcpyAsync(surfaces + (size_t)i * cells, from[i], cells * 8, kind, s));
  }
  stream_sync(s);
  events.read();
  *n_ground = ground;
  PST_API_END
}

int pst_grid_morphology_device(const double* d_in, double* d_out, uint32_t cols, uint32_t rows, uint32_t half_width, uint32_t op) {
  PST_API_BEGIN
  const std::string who = "pst_grid_morphology_device";
  if (op > 1) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": op must be 0 (erode) or 1 (dilate)");
  if (cols == 0 || rows == 0) return PST_OK;
  not_null(d_in, "d_in");
  not_null(d_out, "d_out");
  if (d_in == d_out) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": the operation is not in place");
  if ((uint64_t)cols * rows > kMaxCells) throw Error(PST_ERR_UNSUPPORTED, who + ": more than 2^28 cells");
  ensure_device();
  hipStream_t s = current_stream();
  const size_t cells = (size_t)cols * rows;
  // in -> ... -> d_out through one scratch raster: an even number of passes starts into the scratch, an odd one into d_out
  Scratch scratch;
  double* tmp = scratch.alloc<double>(cells * 8, s, who.c_str());
  Passes passes{cols, rows, {tmp, d_out}, s, d_in, false};
  if (passes.count(half_width) % 2) std::swap(passes.bufs[0], passes.bufs[1]);
  passes.run(half_width, op == 1);
  PST_API_END
}

int pst_finite_mask_device(const pst_buffer* b, uint8_t* d_mask) {
  PST_API_BEGIN
  not_null(b, "buffer");
  const Member& pm = position_member(*b);
  if (b->len == 0) return PST_OK;
  not_null(d_mask, "d_mask");
  ensure_device();
  if (!pstk::finite_mask(positions_of(*b, pm), d_mask, current_stream())) throw hip_failure("finite mask launch failed: ");
  PST_API_END
}

int pst_buffer_set_u8_where_device(pst_buffer* b, const char* attribute_name, const uint8_t* d_mask, uint8_t value) {
  PST_API_BEGIN
  not_null(b, "buffer");
  not_null(attribute_name, "attribute_name");
  const Member& m = required(b->layout.find(AttributeDef{attribute_name, DataType{}}));  // (a default datatype is U8)
  if (b->len == 0) return PST_OK;
  not_null(d_mask, "d_mask");
  ensure_device();
  const AttrView v = attr_view(*b, &m);
  if (!pstk::set_u8_where(v.addr, v.stride, b->len, d_mask, value, current_stream())) throw hip_failure("set-where launch failed: ");
  PST_API_END
}

}  // extern "C"
