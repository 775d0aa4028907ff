// pst_nn_index_* / pst_nearest_neighbours_device / pst_distance_mask_device / pst_icp_step / pst_icp / pst_icp_plane_step / pst_icp_plane /
// pst_nn_kernel_shape: argument checks, the persistent index over a target cloud and its normals, the scratch of a search and the two ICP loops
// around nn.hip (where the definitions and the ring argument are).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "nn_index.hpp"
#include "phase_events.hpp"
#include "plane_solve.hpp"
#include "rigid_solve.hpp"

using namespace pst;

namespace {

// automatic edge: the mean number of targets per OCCUPIED cell is brought into [kMeanLow, kMeanHigh], aiming at kMeanAim
constexpr double kMeanLow = 2.0, kMeanHigh = 16.0, kMeanAim = 6.0;
constexpr double kStopMargin = 0x1p-20;  // edge_stop = edge * (1 - 2^-20), the margin of the ring bound (nn.hip)

// the cluster grid (cluster_grid.hpp) for a given edge, written to *cells for the key kernel; returned with the far corner and the ring
// bound's edge for the searches
pstk::NnGrid make_grid(const FiniteBounds& b, double edge, pstk::ClusterGrid* cells) {
  if (!pstk::cluster_grid_for_edge(b.min, b.max, edge, cells)) throw Error(PST_ERR_UNSUPPORTED, "pst_nn_index_create: the extent of the finite points overflows f64");
  pstk::NnGrid g{};
  for (int a = 0; a < 3; ++a) {
    g.min[a] = cells->min[a];
    g.max[a] = b.max[a];
    g.dim[a] = cells->dim[a];
    g.bits[a] = cells->bits[a];
  }
  g.edge = cells->edge;
  g.edge_stop = g.edge * (1.0 - kStopMargin);
  return g;
}

// First guess of the automatic edge: kMeanAim points per cell if the points filled the box.  An axis whose extent is below the edge that comes
// out holds one layer of cells whatever the edge: it is taken out and the guess repeated over the remaining axes (a slab is gridded as a
// rectangle, a rod as a line).  A sheet that is not axis-parallel still fills a small share of its box, which only the count of occupied
// cells after the sort can tell.
double first_edge(const FiniteBounds& b) {
  double extent[3], longest = 0.0;
  bool active[3];
  for (int a = 0; a < 3; ++a) {
    extent[a] = b.max[a] - b.min[a];
    active[a] = extent[a] > 0.0 && std::isfinite(extent[a]);
    if (active[a]) longest = std::fmax(longest, extent[a]);
  }
  double edge = 1.0;  // every finite point is the same point: one cell whatever the edge
  for (int round = 0; round < 3; ++round) {
    double log_volume = 0.0;
    int axes = 0;
    for (int a = 0; a < 3; ++a)
      if (active[a]) { log_volume += std::log(extent[a]); ++axes; }
    if (axes == 0) break;
    edge = std::exp((log_volume + std::log(kMeanAim / (double)b.count)) / axes);  // (logarithms: the product of the extents may overflow)
    bool dropped = false;
    for (int a = 0; a < 3; ++a)
      if (active[a] && extent[a] < edge && extent[a] < longest) { active[a] = false; dropped = true; }
    if (!dropped) break;
  }
  if (!(edge > longest * 0x1p-40) || !std::isfinite(edge)) edge = longest > 0.0 ? longest * 0x1p-20 : 1.0;
  return edge;
}

struct CheckedTransform {
  pstk::NnTransform t{};
  CheckedTransform(const double* m12, const char* who) {
    t.on = m12 ? 1 : 0;
    if (m12)
      for (int i = 0; i < 12; ++i) {
        if (!std::isfinite(m12[i])) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": the transform has an entry that is not finite");
        t.m[i] = m12[i];
      }
  }
};

thread_local double t_phase_ms[2] = {0.0, 0.0};  // PST_NN_TIMES=1 (tools/bench_nn.py reads them through pst_nn_phase_times)

bool times_wanted() {
  static const bool wanted = env_nonzero("PST_NN_TIMES");
  return wanted;
}

// The search of one query cloud: keys -> sort -> search, in one block of scratch that lives until the caller has synchronised.
struct Search {
  Scratch scratch;
  PhaseEvents<2> events{times_wanted(), t_phase_ms};
  uint32_t* at = nullptr;  // with_at: position of every query's match in the index's sorted arrays
  void run(const pst_nn_index& ix, const pstk::Positions& pos, const pstk::NnTransform& t, double m2, uint32_t* d_idx, double* d_dist, bool with_at, size_t extra_bytes,
           size_t* extra_offset, hipStream_t s, const char* who) {
    const size_t n = pos.n;
    size_t sort_bytes = 0;
    PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
    const bool walk = ix.nf != 0;
    const size_t b4 = up256(n * 4), b8 = up256(n * 8);
    ScratchLayout layout;
    const size_t off_keys_a = layout.add(walk ? b8 : 0), off_keys_b = layout.add(walk ? b8 : 0), off_vals_a = layout.add(walk ? b4 : 0), off_order = layout.add(walk ? b4 : 0);
    const size_t off_tmp = layout.add(walk ? sort_bytes : 0), off_at = layout.add(with_at ? b4 : 0), off_extra = layout.add(extra_bytes);
    if (extra_offset) *extra_offset = off_extra;
    if (layout.total() == 0) layout.add(256);
    scratch.alloc(layout.total(), s, who);
    at = with_at ? scratch.at<uint32_t>(off_at) : nullptr;
    uint64_t* keys_b = nullptr;
    uint32_t* order = nullptr;
    events.mark(0, s);
    if (walk) {
      uint64_t* keys_a = scratch.at<uint64_t>(off_keys_a);
      keys_b = scratch.at<uint64_t>(off_keys_b);
      uint32_t* vals_a = scratch.at<uint32_t>(off_vals_a);
      order = scratch.at<uint32_t>(off_order);
      if (!pstk::nn_query_keys(pos, t, ix.grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure(std::string(who) + ": query key launch failed: ");
      size_t bytes = sort_bytes;
      PST_HIP_CHECK(pstk::sort_pairs_u64(scratch.at<void>(off_tmp), bytes, keys_a, keys_b, vals_a, order, n, ix.grid.bits[0] + ix.grid.bits[1] + ix.grid.bits[2] + 1, s));
    }
    events.mark(1, s);
    if (!pstk::nn_search(pos, t, ix.grid, m2, (const unsigned long long*)keys_b, order, (const unsigned long long*)ix.keys, ix.xs, ix.ys, ix.zs, ix.order, ix.nf, d_idx,
                         d_dist, at, s))
      throw hip_failure(std::string(who) + ": search launch failed: ");
    events.mark(2, s);
  }
};

// One ICP step on checked arguments: sums[17] and T_out; returns the number of matched points.
uint64_t icp_step(const pst_nn_index& ix, const pstk::Positions& pos, const double T_in[12], double m2, double sums[17], double T_out[12], hipStream_t s, const char* who) {
  pstk::NnTransform t{};
  t.on = 1;
  std::memcpy(t.m, T_in, sizeof(t.m));
  pstk::NnSums r{};
  if (pos.n) {
    Search search;
    size_t off = 0;
    const size_t part = up256(pstk::nn_icp_partials_bytes(pos.n));
    search.run(ix, pos, t, m2, nullptr, nullptr, true, part + 256, &off, s, who);
    void* partials = search.scratch.at<void>(off);
    pstk::NnSums* rec = search.scratch.at<pstk::NnSums>(off + part);
    if (!pstk::nn_icp_sums(pos, t, search.at, ix.xs, ix.ys, ix.zs, ix.grid.min, partials, rec, s)) throw hip_failure(std::string(who) + ": reduction launch failed: ");
    PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
    stream_sync(s);
  }
  if (r.matched < 3) throw Error(PST_ERR_TOO_FEW_POINTS, std::string(who) + ": fewer than 3 source points have a match within max_distance");
  sums[0] = (double)r.matched;
  std::memcpy(sums + 1, r.cq, 3 * sizeof(double));
  std::memcpy(sums + 4, r.cp, 3 * sizeof(double));
  std::memcpy(sums + 7, r.H, 9 * sizeof(double));
  sums[16] = r.sum_d2;
  double R[9], dt[3];
  rigid_solve(r.H, r.cq, r.cp, R, dt);
  rigid_compose(R, dt, T_in, T_out);
  return r.matched;
}

// One point-to-plane step on checked arguments (the index has normals): sums[35] and T_out; returns the number of used pairs.
uint64_t icp_plane_step(const pst_nn_index& ix, const pstk::Positions& pos, const double T_in[12], double m2, double sums[35], double T_out[12], hipStream_t s,
                        const char* who) {
  pstk::NnTransform t{};
  t.on = 1;
  std::memcpy(t.m, T_in, sizeof(t.m));
  pstk::NnPlaneSums r{};
  if (pos.n && ix.nf) {  // (no finite target: no normals are held and nothing can match)
    Search search;
    size_t off = 0;
    const size_t part = up256(pstk::nn_plane_partials_bytes(pos.n));
    search.run(ix, pos, t, m2, nullptr, nullptr, true, part + 512, &off, s, who);
    void* partials = search.scratch.at<void>(off);
    pstk::NnPlaneSums* rec = search.scratch.at<pstk::NnPlaneSums>(off + part);
    if (!pstk::nn_plane_sums(pos, t, search.at, ix.xs, ix.ys, ix.zs, ix.nx, ix.ny, ix.nz, ix.grid.min, partials, rec, s))
      throw hip_failure(std::string(who) + ": reduction launch failed: ");
    PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
    stream_sync(s);
  }
  if (r.used < 6) throw Error(PST_ERR_TOO_FEW_POINTS, std::string(who) + ": fewer than 6 source points have a match within max_distance whose normal is finite and not zero");
  sums[0] = (double)r.matched;
  sums[1] = (double)r.used;
  std::memcpy(sums + 2, r.cq, 3 * sizeof(double));
  std::memcpy(sums + 5, r.A, 21 * sizeof(double));
  std::memcpy(sums + 26, r.g, 6 * sizeof(double));
  sums[32] = r.sum_r2;
  sums[33] = r.sum_w2;
  sums[34] = r.sum_d2;
  double dR[9], dt[3];
  plane_solve(r.A, r.g, r.sum_w2, (double)r.used, r.cq, dR, dt);
  rigid_compose(dR, dt, T_in, T_out);
  return r.used;
}

void require_normals(const pst_nn_index& ix, const char* who) {
  if (!ix.has_normals) throw Error(PST_ERR_MISSING_ATTRIBUTE, std::string(who) + ": the index has no normals (pst_nn_index_set_normals, pst_nn_index_set_normals_device)");
}

// The normals at base + i * stride (f64 or f32 triples, target-buffer order) gathered into a new block that replaces the index's.
void set_normals(pst_nn_index& ix, const uint8_t* base, uint64_t stride, bool is_f32, const char* who) {
  if (ix.nf == 0) {  // nothing to hold
    ix.has_normals = true;
    return;
  }
  hipStream_t s = current_stream();
  const size_t f8 = up256((size_t)ix.nf * 8);
  void* block = nullptr;
  PST_HIP_CHECK(dev_malloc_retry(&block, 3 * f8));
  double *nx = (double*)block, *ny = (double*)((uint8_t*)block + f8), *nz = (double*)((uint8_t*)block + 2 * f8);
  const bool launched = pstk::nn_gather_normals(base, stride, is_f32, ix.order, ix.nf, nx, ny, nz, s);
  const hipError_t synced = launched ? hipStreamSynchronize(s) : hipSuccess;  // the source is not read after this call
  if (!launched || synced != hipSuccess) {
    (void)hipFree(block);
    if (!launched) throw hip_failure(std::string(who) + ": gather launch failed: ");
    PST_HIP_CHECK(synced);
  }
  ix.drop_normals();
  ix.normals_block = block;
  ix.nx = nx; ix.ny = ny; ix.nz = nz;
  ix.has_normals = true;
}

}  // namespace

extern "C" {

int pst_nn_kernel_shape(uint32_t* queries_per_block, uint32_t* reduce_block, uint32_t* reduce_points_per_block) {
  if (queries_per_block) *queries_per_block = pstk::kNnQueriesPerBlock;
  if (reduce_block) *reduce_block = pstk::kNnReduceBlock;
  if (reduce_points_per_block) *reduce_points_per_block = pstk::kNnReducePoints;
  return PST_OK;
}

int pst_nn_phase_times(double ms[2]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_nn_index_create(const pst_buffer* target, double cell_edge, pst_nn_index** out) {
  PST_API_BEGIN
  const char* who = "pst_nn_index_create";
  not_null(target, "target");
  not_null(out, "out");
  *out = nullptr;
  if (!(cell_edge >= 0.0) || std::isinf(cell_edge)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": cell_edge must be finite and not negative (0: automatic)");
  const Member& pm = position_member(*target);
  ensure_device();
  check_point_count(target->len, who);
  std::unique_ptr<pst_nn_index> ix(new pst_nn_index);
  const size_t n = target->len;
  ix->n_target = n;
  if (n == 0) {  // an empty target: every query is unmatched
    *out = ix.release();
    return PST_OK;
  }
  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*target, pm);
  size_t sort_bytes = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  const size_t b4 = up256(n * 4), b8 = up256(n * 8);
  ScratchLayout layout;
  const size_t off_keys_a = layout.add(b8), off_keys_b = layout.add(b8), off_vals_a = layout.add(b4), off_order = layout.add(b4);
  const size_t off_rec = layout.add(256), off_count = layout.add(256), off_tmp = layout.add(sort_bytes);
  Scratch scratch(layout, s, who);
  uint64_t* keys_a = scratch.at<uint64_t>(off_keys_a);
  uint64_t* keys_b = scratch.at<uint64_t>(off_keys_b);
  uint32_t* vals_a = scratch.at<uint32_t>(off_vals_a);
  uint32_t* order = scratch.at<uint32_t>(off_order);
  pstk::ClusterRecord* rec = scratch.at<pstk::ClusterRecord>(off_rec);
  unsigned long long* count = scratch.at<unsigned long long>(off_count);

  const FiniteBounds bounds = finite_bounds(pos, rec, s, who);
  const uint32_t nf = (uint32_t)bounds.count;
  if (nf == 0) {  // no finite target
    *out = ix.release();
    return PST_OK;
  }
  // Key, sort, count the occupied cells; with an automatic edge, up to two more rounds while the mean occupancy lies outside the band.  The
  // occupancy goes with edge^d, d the cloud's local dimension: 2 is assumed for the first correction (sheets are what the box volume gets
  // wrong), the second one takes d from the two measurements.
  pstk::NnGrid grid{};
  double edge = cell_edge > 0.0 ? cell_edge : first_edge(bounds), prev_edge = 0.0, prev_mean = 0.0;
  unsigned long long occupied = 0;
  for (int round = 0;; ++round) {
    pstk::ClusterGrid cells{};
    grid = make_grid(bounds, edge, &cells);
    cluster_sorted_keys(pos, cells, keys_a, keys_b, vals_a, order, scratch.at<void>(off_tmp), sort_bytes, s, who);
    if (!pstk::nn_count_cells((const unsigned long long*)keys_b, nf, count, s)) throw hip_failure(std::string(who) + ": cell count launch failed: ");
    PST_HIP_CHECK(hipMemcpyAsync(&occupied, count, sizeof(occupied), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    const double mean = (double)nf / (double)occupied;
    if (cell_edge > 0.0 || round == 2 || (mean >= kMeanLow && mean <= kMeanHigh)) break;
    double d = 2.0;
    if (round == 1 && mean != prev_mean) d = std::fmin(3.0, std::fmax(1.0, std::log(mean / prev_mean) / std::log(grid.edge / prev_edge)));
    const double next = grid.edge * std::pow(kMeanAim / mean, 1.0 / d);
    if (!(next > 0.0) || !std::isfinite(next) || (next < grid.edge && grid.edge != edge)) break;  // (smaller cells than the key width allows: keep these)
    prev_edge = grid.edge;
    prev_mean = mean;
    edge = next;
  }
  // the index's own memory
  const size_t f8 = up256((size_t)nf * 8), f4 = up256((size_t)nf * 4);
  PST_HIP_CHECK(dev_malloc_retry(&ix->block, 4 * f8 + f4));
  uint8_t* base = (uint8_t*)ix->block;
  ix->keys = (uint64_t*)base;
  ix->xs = (double*)(base + f8);
  ix->ys = (double*)(base + 2 * f8);
  ix->zs = (double*)(base + 3 * f8);
  ix->order = (uint32_t*)(base + 4 * f8);
  ix->grid = grid;
  ix->nf = nf;
  ix->occupied = occupied;
  PST_HIP_CHECK(hipMemcpyAsync(ix->keys, keys_b, (size_t)nf * 8, hipMemcpyDeviceToDevice, s));
  PST_HIP_CHECK(hipMemcpyAsync(ix->order, order, (size_t)nf * 4, hipMemcpyDeviceToDevice, s));
  if (!pstk::nn_gather(pos, ix->order, nf, ix->xs, ix->ys, ix->zs, s)) throw hip_failure(std::string(who) + ": gather launch failed: ");
  stream_sync(s);  // the target buffer is not read after this call
  *out = ix.release();
  PST_API_END
}

int pst_nn_index_destroy(pst_nn_index* index) {
  PST_API_BEGIN
  delete index;
  PST_API_END
}

int pst_nn_index_grid(const pst_nn_index* index, double min_and_edge[4], uint32_t dim[3], uint64_t* n_finite, uint64_t* occupied_cells) {
  PST_API_BEGIN
  not_null(index, "index");
  if (min_and_edge) {
    for (int a = 0; a < 3; ++a) min_and_edge[a] = index->grid.min[a];
    min_and_edge[3] = index->grid.edge;
  }
  if (dim)
    for (int a = 0; a < 3; ++a) dim[a] = index->grid.dim[a];
  if (n_finite) *n_finite = index->nf;
  if (occupied_cells) *occupied_cells = index->occupied;
  PST_API_END
}

int pst_nearest_neighbours_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double max_distance, uint32_t* d_idx, double* d_dist) {
  PST_API_BEGIN
  const char* who = "pst_nearest_neighbours_device";
  not_null(index, "index");
  not_null(query, "query");
  if (!d_idx && !d_dist) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": d_idx and d_dist must not both be NULL");
  const double m2 = checked_m2(max_distance, who);
  const CheckedTransform t(transform12, who);
  const Member& pm = position_member(*query);
  ensure_device();
  check_point_count(query->len, who);
  if (query->len == 0) return PST_OK;
  hipStream_t s = current_stream();
  Search search;
  search.run(*index, positions_of(*query, pm), t.t, m2, d_idx, d_dist, false, 0, nullptr, s, who);
  stream_sync(s);
  search.events.read();
  PST_API_END
}

int pst_distance_mask_device(const double* d_dist, uint64_t n, double threshold, int keep_far, uint8_t* d_mask) {
  PST_API_BEGIN
  if (n == 0) return PST_OK;
  not_null(d_dist, "d_dist");
  not_null(d_mask, "d_mask");
  ensure_device();
  if (!pstk::nn_distance_mask(d_dist, n, threshold, keep_far, d_mask, current_stream())) throw hip_failure("distance mask launch failed: ");
  PST_API_END
}

int pst_icp_step(const pst_nn_index* index, const pst_buffer* source, const double T_in[12], double max_distance, double sums[17], double T_out[12]) {
  PST_API_BEGIN
  const char* who = "pst_icp_step";
  not_null(index, "index");
  not_null(source, "source");
  not_null(T_in, "T_in");
  not_null(sums, "sums");
  not_null(T_out, "T_out");
  const double m2 = checked_m2(max_distance, who);
  const CheckedTransform t(T_in, who);
  const Member& pm = position_member(*source);
  ensure_device();
  check_point_count(source->len, who);
  double out[12];
  icp_step(*index, positions_of(*source, pm), t.t.m, m2, sums, out, current_stream(), who);
  std::memcpy(T_out, out, sizeof(out));  // (T_out may be T_in)
  PST_API_END
}

int pst_icp(const pst_nn_index* index, const pst_buffer* source, const double* T_init, double max_distance, uint32_t max_iterations, double rms_tolerance, double T_out[12],
            double* rms, uint64_t* matched, uint32_t* iterations) {
  PST_API_BEGIN
  const char* who = "pst_icp";
  not_null(index, "index");
  not_null(source, "source");
  not_null(T_out, "T_out");
  const double m2 = checked_m2(max_distance, who);
  const CheckedTransform t(T_init, who);
  if (max_iterations == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_iterations must be at least 1");
  if (!(rms_tolerance >= 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": rms_tolerance must not be negative");
  const Member& pm = position_member(*source);
  ensure_device();
  check_point_count(source->len, who);
  const pstk::Positions pos = positions_of(*source, pm);
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, next[12], sums[17];
  if (T_init) std::memcpy(T, T_init, sizeof(T));
  double last_rms = 0.0;
  uint64_t m = 0;
  uint32_t steps = 0;
  // the step function in a loop: stop after the step whose misfit differs from the previous step's by at most the tolerance
  while (steps < max_iterations) {
    m = icp_step(*index, pos, T, m2, sums, next, current_stream(), who);
    std::memcpy(T, next, sizeof(T));
    const double step_rms = std::sqrt(sums[16] / sums[0]);
    ++steps;
    const bool settled = steps > 1 && std::fabs(step_rms - last_rms) <= rms_tolerance;
    last_rms = step_rms;
    if (settled) break;
  }
  std::memcpy(T_out, T, sizeof(T));
  if (rms) *rms = last_rms;
  if (matched) *matched = m;
  if (iterations) *iterations = steps;
  PST_API_END
}

int pst_nn_index_set_normals_device(pst_nn_index* index, const double* d_normals, uint64_t n) {
  PST_API_BEGIN
  const char* who = "pst_nn_index_set_normals_device";
  not_null(index, "index");
  if (!d_normals) {  // drop them
    index->drop_normals();
    return PST_OK;
  }
  if (n != index->n_target) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": n must equal the length the target had when the index was created");
  ensure_device();
  set_normals(*index, (const uint8_t*)d_normals, 24, false, who);
  PST_API_END
}

int pst_nn_index_set_normals(pst_nn_index* index, const pst_buffer* b) {
  PST_API_BEGIN
  const char* who = "pst_nn_index_set_normals";
  not_null(index, "index");
  not_null(b, "buffer");
  if (b->len != index->n_target) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": the buffer's length must equal the length the target had when the index was created");
  AttributeDef nd{"Normal", DataType{}};
  nd.datatype.kind = PST_VEC3F32;
  const Member* nm = b->layout.find(nd);
  if (!nm) throw Error(PST_ERR_MISSING_ATTRIBUTE, std::string(who) + ": the buffer's PointLayout has no Normal (Vec3f32)");
  ensure_device();
  const AttrView v = attr_view(*b, nm);
  set_normals(*index, (const uint8_t*)(uintptr_t)v.addr, v.stride, true, who);
  PST_API_END
}

int pst_nn_index_has_normals(const pst_nn_index* index, int* out) {
  PST_API_BEGIN
  not_null(index, "index");
  not_null(out, "out");
  *out = index->has_normals ? 1 : 0;
  PST_API_END
}

int pst_icp_plane_step(const pst_nn_index* index, const pst_buffer* source, const double T_in[12], double max_distance, double sums[35], double T_out[12]) {
  PST_API_BEGIN
  const char* who = "pst_icp_plane_step";
  not_null(index, "index");
  not_null(source, "source");
  not_null(T_in, "T_in");
  not_null(sums, "sums");
  not_null(T_out, "T_out");
  const double m2 = checked_m2(max_distance, who);
  const CheckedTransform t(T_in, who);
  const Member& pm = position_member(*source);
  require_normals(*index, who);
  ensure_device();
  check_point_count(source->len, who);
  double out[12];
  icp_plane_step(*index, positions_of(*source, pm), t.t.m, m2, sums, out, current_stream(), who);
  std::memcpy(T_out, out, sizeof(out));  // (T_out may be T_in)
  PST_API_END
}

int pst_icp_plane(const pst_nn_index* index, const pst_buffer* source, const double* T_init, double max_distance, uint32_t max_iterations, double rms_tolerance,
                  double T_out[12], double* rms, uint64_t* used, uint32_t* iterations) {
  PST_API_BEGIN
  const char* who = "pst_icp_plane";
  not_null(index, "index");
  not_null(source, "source");
  not_null(T_out, "T_out");
  const double m2 = checked_m2(max_distance, who);
  const CheckedTransform t(T_init, who);
  if (max_iterations == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_iterations must be at least 1");
  if (!(rms_tolerance >= 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": rms_tolerance must not be negative");
  const Member& pm = position_member(*source);
  require_normals(*index, who);
  ensure_device();
  check_point_count(source->len, who);
  const pstk::Positions pos = positions_of(*source, pm);
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, next[12], sums[35];
  if (T_init) std::memcpy(T, T_init, sizeof(T));
  double last_rms = 0.0;
  uint64_t u = 0;
  uint32_t steps = 0;
  // the stopping rule of pst_icp on the point-to-plane misfit sqrt(sum_r2 / u)
  while (steps < max_iterations) {
    u = icp_plane_step(*index, pos, T, m2, sums, next, current_stream(), who);
    std::memcpy(T, next, sizeof(T));
    const double step_rms = std::sqrt(sums[32] / sums[1]);
    ++steps;
    const bool settled = steps > 1 && std::fabs(step_rms - last_rms) <= rms_tolerance;
    last_rms = step_rms;
    if (settled) break;
  }
  std::memcpy(T_out, T, sizeof(T));
  if (rms) *rms = last_rms;
  if (used) *used = u;
  if (iterations) *iterations = steps;
  PST_API_END
}

}  // extern "C"
