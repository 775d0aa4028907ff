// pst_poisson_disk_mask / pst_sample_priorities / pst_sample_kernel_shape / pst_sample_phase_times: argument checks, the scratch layout, the
// loop of decision rounds and the order of the launches of sample.hip (where the definitions and the ordering argument are; the grid is
// cluster_grid.hpp's, the index build cluster_index.hpp's).
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

enum : uint32_t { kShuffled = 0, kIndexOrder = 1 };  // PST_SAMPLE_SHUFFLED, PST_SAMPLE_INDEX_ORDER

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_SAMPLE_TIMES=1 (tools/bench_sample.py reads them through pst_sample_phase_times)

}  // namespace

extern "C" {

int pst_sample_kernel_shape(uint32_t* points_per_block, uint32_t* sweeps_per_launch) {
  if (points_per_block) *points_per_block = pstk::kSamplePointsPerBlock;
  if (sweeps_per_launch) *sweeps_per_launch = pstk::kSampleSweepsPerLaunch;
  return PST_OK;
}

int pst_sample_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_sample_priorities(uint32_t order, uint64_t seed, uint64_t first, uint64_t count, uint64_t* keys) {
  PST_API_BEGIN
  if (order > kIndexOrder) throw Error(PST_ERR_INVALID_ARGUMENT, "pst_sample_priorities: order must be 0 (shuffled) or 1 (index order)");
  if (count == 0) return PST_OK;
  not_null(keys, "keys");
  for (uint64_t j = 0; j < count; ++j) keys[j] = order == kShuffled ? splitmix64(seed ^ (first + j)) : first + j;
  PST_API_END
}

int pst_poisson_disk_mask(const pst_buffer* b, double radius, uint32_t order, uint64_t seed, uint8_t* mask, uint32_t mask_memkind, uint64_t* kept, uint32_t* rounds) {
  PST_API_BEGIN
  const std::string who = "pst_poisson_disk_mask";
  not_null(b, "buffer");
  not_null(mask, "mask");
  not_null(kept, "kept");
  if (mask_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid mask memory kind");
  if (order > kIndexOrder) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": order must be 0 (shuffled) or 1 (index order)");
  const double r2 = radius * radius;
  if (!std::isfinite(radius) || !(radius > 0.0) || !std::isnormal(r2))
    throw Error(PST_ERR_INVALID_ARGUMENT, who + ": radius must be finite and positive, and its square a normal number");
  const Member& pm = position_member(*b);
  ensure_device();
  check_point_count(b->len, who);
  *kept = 0;
  if (rounds) *rounds = 0;
  const size_t n = b->len;
  if (n == 0) return PST_OK;  // no points: nothing kept, no mask byte to write

  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  const bool mask_on_device = mask_memkind == PST_MEM_DEVICE;

  // One block of scratch.  The sort's input pair is dead once the sort has run; the rounds' bookkeeping lives in it:
  //   keys_a (8(n + 1))  unsorted keys     -> the scan's offsets
  //   keys_b (8n)        sorted keys, to the end
  //   vals_a (4n)        unsorted indices  -> one of the two active lists
  //   order  (4n)        buffer index of sorted position s, to the end
  //   xs, ys, zs (8n)    sorted positions
  //   state (n), flags (4(n + 1)), the other active list (4n), bounds partials and record, the kept count, sort / scan scratch, mask (host masks only)
  size_t sort_bytes = 0, scan_bytes = 0;
  PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
  const size_t tmp_bytes = std::max(sort_bytes, scan_bytes);
  ScratchLayout layout;
  ClusterIndex ix;
  ix.carve(layout, n);
  const size_t off_state = layout.add(n), off_flags = layout.add(ix.b4);
  const size_t off_active = layout.add(ix.b4), off_partials = layout.add(pstk::sample_bounds_partials_bytes(n)), off_rec = layout.add(256), off_kept = layout.add(256);
  const size_t off_tmp = layout.add(tmp_bytes), off_mask = layout.add(mask_on_device ? 0 : n);
  Scratch scratch(layout, s, who.c_str());
  ix.bind(scratch);
  uint8_t* state = scratch.at<uint8_t>(off_state);
  uint32_t* flags = scratch.at<uint32_t>(off_flags);
  pstk::SampleBounds* rec = scratch.at<pstk::SampleBounds>(off_rec);
  unsigned long long* kept_dev = scratch.at<unsigned long long>(off_kept);
  void* tmp = scratch.at<void>(off_tmp);
  uint8_t* mask_dev = mask_on_device ? mask : scratch.at<uint8_t>(off_mask);

  static const bool timed = env_nonzero("PST_SAMPLE_TIMES");
  PhaseEvents<3> events(timed, t_phase_ms);
  events.mark(0, s);
  // ---- index build: AABB of the finite points -> (host: grid) -> keys -> sort -> gather
  const FiniteBounds bounds = finite_bounds_folded(pos, scratch.at<void>(off_partials), rec, s, who);
  const uint32_t nf = (uint32_t)bounds.count;
  if (nf == 0) {  // nothing but non-finite points: nothing kept, no round
    fill_result(mask, 0, n, mask_on_device, s);
    stream_sync(s);
    return PST_OK;
  }
  const pstk::ClusterGrid grid = cluster_grid_over(bounds, radius, who);
  ix.build(pos, grid, nf, tmp, tmp_bytes, s, who, true);
  PST_HIP_CHECK(hipMemsetAsync(state, 0, nf, s));  // every point undecided
  PST_HIP_CHECK(hipMemsetAsync(kept_dev, 0, sizeof(*kept_dev), s));
  events.mark(1, s);
  // ---- decision rounds: decide the active points, compact the still undecided ones into the next active list, read back their number.  The
  // undecided point of smallest key decides in every launch, so m falls to 0; there is no cap.
  unsigned long long* offsets = (unsigned long long*)ix.keys_a;
  uint32_t* lists[2] = {ix.vals_a, scratch.at<uint32_t>(off_active)};
  const uint32_t* active = nullptr;  // the first round: every sorted point
  uint32_t m = nf, launches = 0;
  while (m) {
    if (!pstk::sample_decide(ix.sorted_keys(), ix.xs, ix.ys, ix.zs, ix.order, nf, grid, r2, order == kShuffled, seed, active, m, state, flags, s))
      throw hip_failure(who + ": decision launch failed: ");
    ++launches;
    size_t bytes = tmp_bytes;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, flags, offsets, (size_t)m + 1, s));
    uint32_t* next = lists[launches & 1];
    if (!pstk::sample_compact(active, flags, offsets, m, next, s)) throw hip_failure(who + ": compaction launch failed: ");
    unsigned long long left = 0;
    PST_HIP_CHECK(hipMemcpyAsync(&left, offsets + m, sizeof(left), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    if (left >= m) throw Error(PST_ERR_HIP, who + ": a decision round decided nothing");  // (cannot happen: see the head of sample.hip)
    active = next;
    m = (uint32_t)left;
  }
  events.mark(2, s);
  // ---- the mask and the kept count
  if (!pstk::sample_mask(ix.order, state, n, nf, mask_dev, kept_dev, s)) throw hip_failure(who + ": mask launch failed: ");
  events.mark(3, s);
  unsigned long long kept_host = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&kept_host, kept_dev, sizeof(kept_host), hipMemcpyDeviceToHost, s));
  if (!mask_on_device) PST_HIP_CHECK(hipMemcpyAsync(mask, mask_dev, n, hipMemcpyDeviceToHost, s));
  stream_sync(s);
  events.read();
  *kept = kept_host;
  if (rounds) *rounds = launches;
  PST_API_END
}

}  // extern "C"
