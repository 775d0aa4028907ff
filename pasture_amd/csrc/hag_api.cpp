// pst_height_above_ground_device / pst_buffer_u8_equals_mask_device / pst_hag_kernel_shape / pst_hag_phase_times: argument checks, the grid
// (hag_grid.hpp), the scratch layout and the order of the launches of hag.hip (where the definitions and the ring argument are).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "dense_directory.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_HAG_TIMES=1 (tools/bench_hag.py reads them through pst_hag_phase_times)

}  // namespace

extern "C" {

int pst_hag_kernel_shape(uint32_t* queries_per_block, uint32_t* max_k, uint32_t* bounds_points_per_block) {
  if (queries_per_block) *queries_per_block = pstk::kHagQueriesPerBlock;
  if (max_k) *max_k = pstk::kHagMaxK;
  if (bounds_points_per_block) *bounds_points_per_block = pstk::kHagBoundsPointsPerBlock;
  return PST_OK;
}

int pst_hag_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_height_above_ground_device(const pst_buffer* query, const pst_buffer* ground, const uint8_t* d_ground_mask, uint32_t k, double max_distance, double cell_edge,
                                   double* d_hag, double* d_ground_z, uint64_t* n_ground, uint64_t* n_unresolved, double grid_min_and_edge[3], uint32_t grid_dim[2]) {
  PST_API_BEGIN
  const char* who = "pst_height_above_ground_device";
  not_null(query, "query");
  not_null(ground, "ground");
  if (!d_hag && !d_ground_z) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": d_hag and d_ground_z must not both be NULL");
  if (k == 0 || k > pstk::kHagMaxK) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": k must be between 1 and 32");
  const double m2 = checked_m2(max_distance, who);
  if (!(cell_edge >= 0.0) || std::isinf(cell_edge)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": cell_edge must be finite and not negative (0: automatic)");
  const Member& qm = position_member(*query);
  const Member& gm = position_member(*ground);
  if (n_ground) *n_ground = 0;
  if (n_unresolved) *n_unresolved = 0;
  if (grid_min_and_edge) grid_min_and_edge[0] = grid_min_and_edge[1] = grid_min_and_edge[2] = 0.0;
  if (grid_dim) grid_dim[0] = grid_dim[1] = 0;
  const size_t nq = query->len, ng_points = ground->len;
  if (nq == 0) return PST_OK;  // no query: nothing to write
  ensure_device();
  check_point_count(nq, who);
  check_point_count(ng_points, who);

  hipStream_t s = current_stream();
  const pstk::Positions qpos = positions_of(*query, qm), gpos = positions_of(*ground, gm);
  static const bool timed = env_nonzero("PST_HAG_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  events.mark(0, s);
  pstk::HagBounds bounds{};
  if (ng_points) bounds = finite_bounds_2d(gpos, d_ground_mask, s, who);  // of G
  const uint32_t ng = (uint32_t)bounds.count;
  unsigned long long unresolved = 0;

  if (ng == 0) {  // no ground: NaN everywhere, every finite query is unresolved, a zero grid
    Scratch block;
    unsigned long long* count = block.alloc<unsigned long long>(256, s, who);
    PST_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(*count), s));
    for (int i = 1; i < 3; ++i) events.mark(i, s);
    if (!pstk::hag_fill_unresolved(qpos, d_hag, d_ground_z, count, s)) throw hip_failure(std::string(who) + ": fill launch failed: ");
    events.mark(3, s);
    PST_HIP_CHECK(hipMemcpyAsync(&unresolved, count, sizeof(unresolved), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    events.read();
    if (n_unresolved) *n_unresolved = unresolved;
    return PST_OK;
  }

  pstk::HagGrid grid{};
  const double edge = cell_edge > 0.0 ? cell_edge : pstk::hag_auto_edge(ng, bounds.max_x - bounds.min_x, bounds.max_y - bounds.min_y, k);
  if (!pstk::hag_make_grid(bounds.min_x, bounds.min_y, bounds.max_x, bounds.max_y, edge, &grid))
    throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": the extent of the ground points overflows f64");
  const size_t cells = (size_t)grid.dim[0] * grid.dim[1];

  // One block of scratch.  The three arrays the directory's sort alternates between serve the query sort afterwards (the gather and the
  // directory are done with them by then, in stream order), so each has max(len(ground), len(query)) words; then x | y | z of G | the query
  // order | sort and scan scratch | the unresolved count.  ix.order = the ground-buffer index of every sorted position.
  ScratchLayout layout;
  DenseDirectory ix;
  ix.carve(layout, packed_keys(grid), cells, ng_points, std::max(nq, ng_points), s);
  size_t sort_q = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_q, nullptr, nullptr, nullptr, nullptr, nq, ix.keys.bits, s));
  const size_t off_xs = layout.add((size_t)ng * 8), off_ys = layout.add((size_t)ng * 8), off_zs = layout.add((size_t)ng * 8);
  const size_t off_qorder = layout.add(nq * 4), off_tmp = layout.add(std::max(ix.tmp_bytes(), sort_q)), off_count = layout.add(256);
  Scratch scratch(layout, s, who);
  ix.bind(scratch);
  uint32_t* qorder = scratch.at<uint32_t>(off_qorder);
  double *xs = scratch.at<double>(off_xs), *ys = scratch.at<double>(off_ys), *zs = scratch.at<double>(off_zs);
  void* tmp = scratch.at<void>(off_tmp);
  unsigned long long* count = scratch.at<unsigned long long>(off_count);

  // ---- the ground index: the heads kernel looks at the ng members alone
  PST_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(*count), s));
  ix.build(ng, tmp, s, who,
           [&](uint32_t* keys) { if (!pstk::hag_ground_keys(gpos, d_ground_mask, grid, keys, s)) throw hip_failure(std::string(who) + ": key launch failed: "); },
           [&] { if (!pstk::nn_gather(gpos, ix.order, ng, xs, ys, zs, s)) throw hip_failure(std::string(who) + ": gather launch failed: "); });
  events.mark(1, s);
  // ---- the queries in cell order
  if (!pstk::hag_query_keys(qpos, grid, ix.keys_a, ix.vals_a, s)) throw hip_failure(std::string(who) + ": query key launch failed: ");
  size_t bytes = sort_q;
  PST_HIP_CHECK(pstk::sort_pairs_u32(tmp, bytes, ix.keys_a, ix.keys_b, ix.vals_a, qorder, nq, ix.keys.bits, s));
  events.mark(2, s);
  // ---- the search
  if (!pstk::hag_search(qpos, grid, k, m2, ix.keys_b, qorder, ix.dir, xs, ys, zs, ix.order, d_hag, d_ground_z, count, s)) throw hip_failure(std::string(who) + ": search launch failed: ");
  events.mark(3, s);
  PST_HIP_CHECK(hipMemcpyAsync(&unresolved, count, sizeof(unresolved), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  if (n_ground) *n_ground = ng;
  if (n_unresolved) *n_unresolved = unresolved;
  if (grid_min_and_edge) { grid_min_and_edge[0] = grid.min[0]; grid_min_and_edge[1] = grid.min[1]; grid_min_and_edge[2] = grid.edge; }
  if (grid_dim) { grid_dim[0] = grid.dim[0]; grid_dim[1] = grid.dim[1]; }
  PST_API_END
}

int pst_buffer_u8_equals_mask_device(const pst_buffer* b, const char* attribute_name, uint8_t value, uint8_t* d_mask) {
  PST_API_BEGIN
  not_null(b, "buffer");
  not_null(attribute_name, "attribute_name");
  const Member& m = required(b->layout.find(AttributeDef{attribute_name, DataType{}}));  // (a default datatype is U8)
  if (b->len == 0) return PST_OK;
  not_null(d_mask, "d_mask");
  ensure_device();
  const AttrView v = attr_view(*b, &m);
  if (!pstk::u8_equals_mask(v.addr, v.stride, b->len, value, d_mask, current_stream())) throw hip_failure("equals-mask launch failed: ");
  PST_API_END
}

}  // extern "C"
