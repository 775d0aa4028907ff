// pst_rasterize / pst_grid_fill_device / pst_raster_kernel_shape / pst_raster_phase_times: argument checks, the grid, the choice between the
// atomic and the sorted path, the scratch layout and the order of the launches of raster.hip (where the definitions are).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "dense_directory.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

constexpr uint64_t kMaxCells = 1ull << 28;

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_RASTER_TIMES=1 (tools/bench_raster.py reads them through pst_raster_phase_times)

// one plane per set bit of `stats`, in ascending bit order, rows x cols doubles each from `base`
pstk::RasterPlanes planes_at(double* base, uint32_t stats, size_t cells) {
  double* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t at = 0;
  for (int bit = 0; bit < 5; ++bit)
    if (stats & (1u << bit)) p[bit] = base + (at++) * cells;
  return pstk::RasterPlanes{p[0], p[1], p[2], p[3], p[4]};
}

}  // namespace

extern "C" {

int pst_raster_kernel_shape(uint32_t* points_per_block, uint32_t* chunk, uint32_t* fill_tile_cols, uint32_t* fill_tile_rows, uint32_t* fill_max_half_width) {
  if (points_per_block) *points_per_block = pstk::kRasterPointsPerBlock;
  if (chunk) *chunk = pstk::kRasterChunk;
  if (fill_tile_cols) *fill_tile_cols = pstk::kPmfTileCols;
  if (fill_tile_rows) *fill_tile_rows = pstk::kPmfTileRows;
  if (fill_max_half_width) *fill_max_half_width = pstk::kRasterFillMaxHalfWidth;
  return PST_OK;
}

int pst_raster_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_rasterize(const pst_buffer* b, const double* d_values, const uint8_t* d_mask, double cell_size, const double origin[2], const uint32_t dim[2], uint32_t stats, double* out,
                  uint32_t out_memkind, double origin_out[2], uint32_t dim_out[2], uint64_t* n_members) {
  PST_API_BEGIN
  const char* who = "pst_rasterize";
  not_null(b, "buffer");
  not_null(out, "out");
  not_null(n_members, "n_members");
  if (out_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid out memory kind");
  if (!std::isfinite(cell_size) || !(cell_size > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": cell_size must be finite and positive");
  if (stats == 0 || stats > 31) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": stats must be a non-empty set of the bits 1 (count), 2 (min), 4 (max), 8 (mean), 16 (variance)");
  if ((origin == nullptr) != (dim == nullptr)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": origin and dim must be given together or not at all");
  const bool given = origin != nullptr;
  pstk::PmfGrid grid{};
  if (given) {
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1])) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": origin must be finite");
    if (dim[0] == 0 || dim[1] == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": dim must not hold a zero");
    if ((uint64_t)dim[0] * dim[1] > kMaxCells) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": the raster would have more than 2^28 cells: use a larger cell_size");
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
  static const bool timed = env_nonzero("PST_RASTER_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  events.mark(0, s);
  if (!given) {
    const pstk::HagBounds r = finite_bounds_2d(pos, nullptr, s, who);  // of the finite points, whatever the mask says
    if (r.count == 0) return PST_OK;  // nothing but non-finite points: no grid, `out` untouched
    grid = pmf_grid_over(r.min_x, r.min_y, r.max_x, r.max_y, cell_size, who);
  }
  events.mark(1, s);
  const size_t cells = (size_t)grid.cols * grid.rows;
  const uint32_t n_planes = (uint32_t)__builtin_popcount(stats);
  const bool out_on_device = out_memkind == PST_MEM_DEVICE;
  const bool sorted = n != 0 && (stats & (pstk::RS_MEAN | pstk::RS_VARIANCE)) != 0;
  const pstk::RasterInput in{d_values, d_mask};
  unsigned long long members = 0;
  uint32_t members_u32 = 0;

  ScratchLayout layout;
  const size_t off_stage = layout.add(out_on_device ? 0 : cells * 8 * n_planes);
  if (!sorted) {
    // the planes (host results only) | min keys | max keys | counts, each only with its plane | the member count
    const size_t off_min = layout.add(stats & pstk::RS_MIN ? cells * 8 : 0), off_max = layout.add(stats & pstk::RS_MAX ? cells * 8 : 0);
    const size_t off_counts = layout.add(stats & pstk::RS_COUNT ? cells * 4 : 0), off_members = layout.add(256);
    Scratch scratch(layout, s, who);
    const pstk::RasterPlanes planes = planes_at(out_on_device ? out : scratch.at<double>(off_stage), stats, cells);
    unsigned long long* min_keys = stats & pstk::RS_MIN ? scratch.at<unsigned long long>(off_min) : nullptr;
    unsigned long long* max_keys = stats & pstk::RS_MAX ? scratch.at<unsigned long long>(off_max) : nullptr;
    uint32_t* counts = stats & pstk::RS_COUNT ? scratch.at<uint32_t>(off_counts) : nullptr;
    unsigned long long* count = scratch.at<unsigned long long>(off_members);
    events.mark(2, s);
    if (n == 0) {  // a caller's grid over no points: every cell empty
      if (!pstk::raster_fill_empty(planes, cells, s)) throw hip_failure(std::string(who) + ": fill launch failed: ");
    } else {
      if (min_keys) PST_HIP_CHECK(hipMemsetAsync(min_keys, 0xFF, cells * 8, s));  // all ones: empty
      if (max_keys) PST_HIP_CHECK(hipMemsetAsync(max_keys, 0, cells * 8, s));     // zero: empty
      if (counts) PST_HIP_CHECK(hipMemsetAsync(counts, 0, cells * 4, s));
      PST_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(*count), s));
      if (!pstk::raster_atomic(pos, in, grid, min_keys, max_keys, counts, count, s)) throw hip_failure(std::string(who) + ": raster launch failed: ");
      if (!pstk::raster_atomic_decode(min_keys, max_keys, counts, cells, planes, s)) throw hip_failure(std::string(who) + ": decode launch failed: ");
      PST_HIP_CHECK(hipMemcpyAsync(&members, count, sizeof(members), hipMemcpyDeviceToHost, s));
    }
    events.mark(3, s);
    if (!out_on_device) PST_HIP_CHECK(hipMemcpyAsync(out, scratch.at<double>(off_stage), cells * 8 * n_planes, hipMemcpyDeviceToHost, s));
    stream_sync(s);
  } else {
    // the planes (host results only) | the directory, ix.order = the buffer index of every sorted position | the values in sorted order | the
    // heavy cells | their number | their chunk partials | sort and scan scratch
    const unsigned cell_bits = pstk::bits_for(cells);
    const uint32_t nonmember_key = 1u << cell_bits;  // at most 2^28
    DenseDirectory ix;
    ix.carve(layout, plain_keys(cell_bits + 1), cells, n, n, s);
    const size_t off_values = layout.add(n * 8), off_heavy = layout.add((n / (pstk::kRasterChunk + 1) + 1) * 4);
    const size_t off_heavy_count = layout.add(256), off_partials = layout.add(pstk::raster_partials_bytes(n)), off_tmp = layout.add(ix.tmp_bytes());
    Scratch scratch(layout, s, who);
    ix.bind(scratch);
    const pstk::RasterPlanes planes = planes_at(out_on_device ? out : scratch.at<double>(off_stage), stats, cells);
    uint32_t *dir = ix.dir, *heavy = scratch.at<uint32_t>(off_heavy), *heavy_count = scratch.at<uint32_t>(off_heavy_count);
    double *values = scratch.at<double>(off_values), *partials = scratch.at<double>(off_partials);
    // ---- keys, sort, directory
    PST_HIP_CHECK(hipMemsetAsync(heavy_count, 0, sizeof(*heavy_count), s));
    ix.build(scratch.at<void>(off_tmp), s, who, [&](uint32_t* keys) {
      if (!pstk::raster_keys(pos, in, grid, nonmember_key, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: ");
    });
    events.mark(2, s);
    // ---- reduction and output
    if (!pstk::raster_gather(pos, in, ix.order, dir, (uint32_t)cells, values, s)) throw hip_failure(std::string(who) + ": gather launch failed: ");
    if (!pstk::raster_reduce(values, dir, (uint32_t)cells, stats, planes, heavy, heavy_count, s)) throw hip_failure(std::string(who) + ": reduction launch failed: ");
    if (!pstk::raster_reduce_heavy(values, dir, (uint32_t)n, (uint32_t)cells, stats, planes, heavy, heavy_count, partials, s))
      throw hip_failure(std::string(who) + ": heavy-cell launch failed: ");
    events.mark(3, s);
    PST_HIP_CHECK(hipMemcpyAsync(&members_u32, dir + cells, sizeof(members_u32), hipMemcpyDeviceToHost, s));
    if (!out_on_device) PST_HIP_CHECK(hipMemcpyAsync(out, scratch.at<double>(off_stage), cells * 8 * n_planes, hipMemcpyDeviceToHost, s));
    stream_sync(s);
    members = members_u32;
  }
  events.read();
  report(grid);
  *n_members = members;
  PST_API_END
}

int pst_grid_fill_device(const double* d_in, double* d_out, uint32_t cols, uint32_t rows, uint32_t half_width) {
  PST_API_BEGIN
  const std::string who = "pst_grid_fill_device";
  if (half_width > pstk::kRasterFillMaxHalfWidth) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": half_width must not exceed 16 (an inverse-distance fill does not compose from smaller ones)");
  if (cols == 0 || rows == 0) return PST_OK;
  not_null(d_in, "d_in");
  not_null(d_out, "d_out");
  if (d_in == d_out) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": the operation is not in place");
  if ((uint64_t)cols * rows > kMaxCells) throw Error(PST_ERR_UNSUPPORTED, who + ": more than 2^28 cells");
  ensure_device();
  hipStream_t s = current_stream();
  if (half_width == 0) {
    PST_HIP_CHECK(hipMemcpyAsync(d_out, d_in, (size_t)cols * rows * 8, hipMemcpyDeviceToDevice, s));
  } else if (!pstk::raster_grid_fill(d_in, d_out, cols, rows, half_width, s)) {
    throw hip_failure(who + ": fill launch failed: ");
  }
  PST_API_END
}

}  // extern "C"
