// pst_m3c2_device / pst_m3c2_kernel_shape / pst_m3c2_phase_times / pst_m3c2_work: argument checks, the scratch and the order of the launches
// around m3c2.hip (where the definitions and the argument of the cull are).
#include <cmath>
#include <cstring>

#include "nn_index.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

constexpr uint32_t kKnownFlags = PST_M3C2_ORIENT_UP;

// in the order the launches run: core keys + sort, normal lookup, cylinder pass; pst_m3c2_phase_times reports the lookup first
thread_local double t_run_ms[3] = {0.0, 0.0, 0.0};
thread_local uint64_t t_work[3] = {0, 0, 0};

bool times_wanted() {
  static const bool wanted = env_nonzero("PST_M3C2_TIMES");
  return wanted;
}
bool work_wanted() {
  static const bool wanted = env_nonzero("PST_M3C2_WORK");
  return wanted;
}

pstk::M3c2Cloud cloud_of(const pst_nn_index& ix) {
  return pstk::M3c2Cloud{(const unsigned long long*)ix.keys, ix.xs, ix.ys, ix.zs, ix.nf, ix.grid};
}

}  // namespace

extern "C" {

int pst_m3c2_kernel_shape(uint32_t* cores_per_block, uint32_t* lanes_per_core) {
  if (cores_per_block) *cores_per_block = pstk::kM3c2CoresPerBlock;
  if (lanes_per_core) *lanes_per_core = pstk::kM3c2LanesPerCore;
  return PST_OK;
}

int pst_m3c2_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  ms[0] = t_run_ms[1];
  ms[1] = t_run_ms[0];
  ms[2] = t_run_ms[2];
  PST_API_END
}

int pst_m3c2_work(uint64_t out[3]) {
  PST_API_BEGIN
  not_null(out, "out");
  std::memcpy(out, t_work, sizeof(t_work));
  PST_API_END
}

int pst_m3c2_device(const pst_nn_index* reference, const pst_nn_index* compared, const pst_buffer* core, const double* d_normals, double radius, double max_depth,
                    uint32_t min_points, double registration_error, uint32_t flags, double* d_distance, double* d_lod, uint8_t* d_significant, uint32_t* d_counts,
                    double* d_sums, double* d_unit_normals, uint64_t* n_significant) {
  PST_API_BEGIN
  const char* who = "pst_m3c2_device";
  not_null(reference, "reference");
  not_null(compared, "compared");
  not_null(core, "core");
  if (!std::isfinite(radius) || !(radius > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": radius must be finite and positive");
  if (!std::isfinite(max_depth) || !(max_depth > 0.0)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_depth must be finite and positive");
  if (!std::isfinite(registration_error) || !(registration_error >= 0.0))
    throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": registration_error must be finite and not negative");
  if (min_points == 0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": min_points must be at least 1");
  if (flags & ~kKnownFlags) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown flag bits");
  if (core->len > 0xFFFFFFFFull) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": more than 2^32 - 1 core points");
  if (!d_distance && !d_lod && !d_significant && !d_counts && !d_sums && !d_unit_normals && !n_significant)
    throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": at least one output must be given");
  const Member& pm = position_member(*core);
  if (!d_normals && !reference->has_normals)
    throw Error(PST_ERR_MISSING_ATTRIBUTE, std::string(who) + ": d_normals is NULL and the reference index has no normals (pst_nn_index_set_normals, pst_nn_index_set_normals_device)");
  ensure_device();
  check_point_count(core->len, who);
  std::memset(t_work, 0, sizeof(t_work));
  if (n_significant) *n_significant = 0;
  const size_t n = core->len;
  if (n == 0) {
    std::memset(t_run_ms, 0, sizeof(t_run_ms));
    return PST_OK;
  }
  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*core, pm);
  // the core points are taken in the order of their cells in the reference grid (in the compared one when the reference has no finite point)
  const pst_nn_index* by = reference->nf ? reference : (compared->nf ? compared : nullptr);
  const bool lookup = !d_normals && reference->nf != 0;  // (no finite reference point: no nearest point, every core point is invalid)
  size_t sort_bytes = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  const size_t b4 = up256(n * 4), b8 = up256(n * 8);
  ScratchLayout layout;
  const size_t off_keys_a = layout.add(by ? b8 : 0), off_keys_b = layout.add(by ? b8 : 0), off_vals_a = layout.add(by ? b4 : 0), off_order = layout.add(by ? b4 : 0);
  const size_t off_tmp = layout.add(by ? sort_bytes : 0), off_at = layout.add(lookup ? b4 : 0), off_counters = layout.add(256);
  Scratch scratch(layout, s, who);
  PhaseEvents<3> events{times_wanted(), t_run_ms};
  uint64_t* keys_b = nullptr;
  uint32_t* order = nullptr;
  const pstk::NnTransform identity{};  // on == 0: the core points as they are stored
  events.mark(0, s);
  if (by) {
    uint64_t* keys_a = scratch.at<uint64_t>(off_keys_a);
    keys_b = scratch.at<uint64_t>(off_keys_b);
    uint32_t* vals_a = scratch.at<uint32_t>(off_vals_a);
    order = scratch.at<uint32_t>(off_order);
    if (!pstk::nn_query_keys(pos, identity, by->grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure(std::string(who) + ": core key launch failed: ");
    size_t bytes = sort_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u64(scratch.at<void>(off_tmp), bytes, keys_a, keys_b, vals_a, order, n, by->grid.bits[0] + by->grid.bits[1] + by->grid.bits[2] + 1, s));
  }
  events.mark(1, s);
  uint32_t* at = nullptr;
  if (lookup) {  // the match of pst_nearest_neighbours_device with unbounded distance and no transform, as its position in the index
    at = scratch.at<uint32_t>(off_at);
    if (!pstk::nn_search(pos, identity, reference->grid, HUGE_VAL, (const unsigned long long*)keys_b, order, (const unsigned long long*)reference->keys, reference->xs,
                         reference->ys, reference->zs, reference->order, reference->nf, nullptr, nullptr, at, s))
      throw hip_failure(std::string(who) + ": normal lookup launch failed: ");
  }
  events.mark(2, s);
  unsigned long long* counters = scratch.at<unsigned long long>(off_counters);
  pstk::M3c2Args a{};
  a.core_base = pos.base;
  a.core_stride = pos.stride;
  a.n = (uint32_t)n;
  a.order = order;
  a.normals = d_normals;
  a.at = at;
  a.nx = reference->nx; a.ny = reference->ny; a.nz = reference->nz;
  a.cloud[0] = cloud_of(*reference);
  a.cloud[1] = cloud_of(*compared);
  a.radius = radius;
  a.max_depth = max_depth;
  a.radius2 = radius * radius;
  a.registration_error = registration_error;
  a.min_points = min_points;
  a.flags = flags;
  a.distance = d_distance; a.lod = d_lod; a.significant = d_significant; a.counts = d_counts; a.sums = d_sums; a.unit_normals = d_unit_normals;
  a.n_significant = counters;
  a.work = work_wanted() ? counters + 1 : nullptr;
  if (!pstk::m3c2_run(a, s)) throw hip_failure(std::string(who) + ": cylinder launch failed: ");
  events.mark(3, s);
  unsigned long long host[4] = {0, 0, 0, 0};
  PST_HIP_CHECK(hipMemcpyAsync(host, counters, a.work ? sizeof(host) : sizeof(host[0]), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  if (n_significant) *n_significant = host[0];
  for (int k = 0; k < 3; ++k) t_work[k] = host[1 + k];
  PST_API_END
}

}  // extern "C"
