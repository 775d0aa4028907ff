// pst_radius_neighbour_counts_device / pst_radius_search_device / pst_radius_kernel_shape / pst_radius_phase_times: argument checks, the
// scratch layout and the order of the launches of radius.hip (where the definitions and the cull's argument are).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cluster_index.hpp"
#include "nn_index.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};  // PST_RADIUS_TIMES=1 (tools/bench_radius.py reads them through pst_radius_phase_times)

// PST_RADIUS_SORT_CAP=<c>: lists of more than min(c, kRadiusSortCap) entries take the path of the long ones (0: every list does) -- the A/B
// switch of the two ordering paths
uint32_t sort_cap() {
  static const long v = env_long("PST_RADIUS_SORT_CAP", pstk::kRadiusSortCap);
  return (uint32_t)std::min<long>(std::max<long>(v, 0), pstk::kRadiusSortCap);
}

struct Checked {
  double r2;
  pstk::NnTransform t{};
  const Member* pm;
};

// the checks both entry points share after their own NULL checks, in the documented order
Checked checked(const pst_buffer& query, const double* transform12, double radius, const std::string& who) {
  Checked c;
  c.r2 = radius * radius;
  if (!std::isfinite(radius) || !(radius > 0.0) || !std::isnormal(c.r2))
    throw Error(PST_ERR_INVALID_ARGUMENT, who + ": radius must be finite and positive, and its square a normal number");
  c.t.on = transform12 ? 1 : 0;
  if (transform12)
    for (int i = 0; i < 12; ++i) {
      if (!std::isfinite(transform12[i])) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": the transform has an entry that is not finite");
      c.t.m[i] = transform12[i];
    }
  c.pm = &position_member(query);
  return c;
}

// The body of both calls.  d_counts nullable; d_offsets nullable (the counts call without a caller's array scans in scratch).  fill: the
// lists are wanted.  Returns the total; throws PST_ERR_UNSUPPORTED and PST_ERR_RANGE after offsets and *total have been written.
void search(const pst_nn_index& ix, const pstk::Positions& pos, const Checked& c, double radius, uint32_t* d_counts, uint64_t* d_offsets, bool fill, uint32_t* d_indices,
            double* d_distances, uint64_t capacity, uint64_t* total_out, hipStream_t s, const std::string& who_s) {
  const char* who = who_s.c_str();
  static const bool timed = env_nonzero("PST_RADIUS_TIMES");
  PhaseEvents<4> events(timed, t_phase_ms);
  const size_t n = pos.n;
  const bool walk = ix.nf != 0 && n != 0;

  // keys a | keys b | order a | the order = the buffer index of every cell-ordered query | counts (n + 1) | offsets (n + 1, unless the
  // caller gave them) | sort and scan scratch
  size_t sort_bytes = 0, scan_bytes = 0;
  if (walk) PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, 64, s));
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, n + 1, s));
  ScratchLayout layout;
  const size_t off_keys_a = layout.add(walk ? n * 8 : 0), off_keys_b = layout.add(walk ? n * 8 : 0), off_vals_a = layout.add(walk ? n * 4 : 0);
  const size_t off_order = layout.add(walk ? n * 4 : 0), off_counts = layout.add((n + 1) * 4), off_offsets = layout.add(d_offsets ? 0 : (n + 1) * 8);
  const size_t off_tmp = layout.add(std::max(sort_bytes, scan_bytes));
  Scratch scratch(layout, s, who);
  uint32_t* counts = scratch.at<uint32_t>(off_counts);
  unsigned long long* offsets = d_offsets ? (unsigned long long*)d_offsets : scratch.at<unsigned long long>(off_offsets);
  void* tmp = scratch.at<void>(off_tmp);

  pstk::RadiusSearch a{};
  a.pos = pos; a.t = c.t; a.g = ix.grid; a.radius = radius; a.r2 = c.r2;
  a.keys = (const unsigned long long*)ix.keys; a.xs = ix.xs; a.ys = ix.ys; a.zs = ix.zs; a.target_index = ix.order; a.nf = ix.nf;

  // ---- query keys and their sort
  events.mark(0, s);
  if (walk) {
    uint64_t *keys_a = scratch.at<uint64_t>(off_keys_a), *keys_b = scratch.at<uint64_t>(off_keys_b);
    uint32_t *vals_a = scratch.at<uint32_t>(off_vals_a), *order = scratch.at<uint32_t>(off_order);
    if (!pstk::nn_query_keys(pos, c.t, ix.grid, (unsigned long long*)keys_a, vals_a, s)) throw hip_failure(who_s + ": query key launch failed: ");
    size_t bytes = sort_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u64(tmp, bytes, keys_a, keys_b, vals_a, order, n, ix.grid.bits[0] + ix.grid.bits[1] + ix.grid.bits[2] + 1, s));
    a.query_keys = (const unsigned long long*)keys_b;
    a.query_order = order;
  }
  events.mark(1, s);
  // ---- count and scan; the total is the call's one host wait
  if (walk) {
    PST_HIP_CHECK(hipMemsetAsync(counts + n, 0, 4, s));
    if (!pstk::radius_count(a, counts, s)) throw hip_failure(who_s + ": count launch failed: ");
  } else {
    PST_HIP_CHECK(hipMemsetAsync(counts, 0, (n + 1) * 4, s));  // no finite target, or no query
  }
  size_t bytes = scan_bytes;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(tmp, bytes, counts, offsets, n + 1, s));
  if (d_counts && n) PST_HIP_CHECK(hipMemcpyAsync(d_counts, counts, n * 4, hipMemcpyDeviceToDevice, s));
  unsigned long long total = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&total, offsets + n, sizeof(total), hipMemcpyDeviceToHost, s));
  events.mark(2, s);
  stream_sync(s);
  if (total_out) *total_out = total;
  const auto finish = [&] {
    events.mark(3, s);
    events.mark(4, s);
    stream_sync(s);
    events.read();
  };
  if (!fill || (d_indices == nullptr && capacity == 0)) {  // the counts call, the counting form
    finish();
    return;
  }
  if (total >= 0xFFFFFFF0ull) throw Error(PST_ERR_UNSUPPORTED, who_s + ": more than 2^32 - 17 neighbours in all: search the queries in parts");
  if (total > capacity) throw Error(PST_ERR_RANGE, who_s + ": the lists hold " + std::to_string(total) + " entries, more than capacity: size the arrays from total and call again");
  if (total == 0) {
    finish();
    return;
  }

  // ---- fill: the d2 keys of the entries | the long lists, their lengths, the lengths' exclusive sum, their number | scan scratch
  const uint32_t cap = sort_cap();
  const size_t long_capacity = (size_t)std::min<uint64_t>(total / ((uint64_t)cap + 1), n) + 1;
  size_t long_scan_bytes = 0;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(nullptr, long_scan_bytes, nullptr, nullptr, long_capacity + 1, s));
  ScratchLayout el;
  const size_t off_d2 = el.add((size_t)total * 8), off_long = el.add((long_capacity + 1) * 4), off_long_size = el.add((long_capacity + 1) * 4);
  const size_t off_long_offset = el.add((long_capacity + 1) * 8), off_long_count = el.add(256), off_ltmp = el.add(long_scan_bytes);
  Scratch entries(el, s, who);
  unsigned long long* d2_keys = entries.at<unsigned long long>(off_d2);
  uint32_t *long_list = entries.at<uint32_t>(off_long), *long_size = entries.at<uint32_t>(off_long_size), *long_count = entries.at<uint32_t>(off_long_count);
  unsigned long long* long_offset = entries.at<unsigned long long>(off_long_offset);
  if (!pstk::radius_fill(a, offsets, d_indices, d2_keys, s)) throw hip_failure(who_s + ": fill launch failed: ");
  events.mark(3, s);
  // ---- order: the short lists in LDS, the long ones through the radix sorts
  PST_HIP_CHECK(hipMemsetAsync(long_count, 0, 4, s));
  if (!pstk::radius_list_long(offsets, (uint32_t)n, cap, long_list, long_size, long_count, s)) throw hip_failure(who_s + ": list launch failed: ");
  if (!pstk::radius_order_short(offsets, (uint32_t)n, total, cap, d_indices, d2_keys, d_distances, s)) throw hip_failure(who_s + ": window launch failed: ");
  uint32_t n_long = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&n_long, long_count, sizeof(n_long), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  if (n_long) {
    unsigned long long listed = 0;  // (n_long <= long_capacity: that many lists of more than cap entries there can be)
    PST_HIP_CHECK(hipMemsetAsync(long_size + n_long, 0, 4, s));
    bytes = long_scan_bytes;
    PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(entries.at<void>(off_ltmp), bytes, long_size, long_offset, (size_t)n_long + 1, s));
    PST_HIP_CHECK(hipMemcpyAsync(&listed, long_offset + n_long, sizeof(listed), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    const size_t L = (size_t)listed;  // <= total
    const unsigned owner_bits = pstk::bits_for(n_long);
    size_t sort64_bytes = 0, sort32_bytes = 0, sort_owner_bytes = 0;
    PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort64_bytes, nullptr, nullptr, nullptr, nullptr, L, 64, s));
    PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort32_bytes, nullptr, nullptr, nullptr, nullptr, L, 32, s, true));
    PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_owner_bytes, nullptr, nullptr, nullptr, nullptr, L, owner_bits, s));
    // the entries' indices | d2 keys | owners | 32-bit sort keys a | b | 64-bit sort keys a | b | slots a | b | sort scratch
    ScratchLayout hl;
    const size_t off_idx = hl.add(L * 4), off_key = hl.add(L * 8), off_owner = hl.add(L * 4), off_k32a = hl.add(L * 4), off_k32b = hl.add(L * 4);
    const size_t off_k64a = hl.add(L * 8), off_k64b = hl.add(L * 8), off_sa = hl.add(L * 4), off_sb = hl.add(L * 4);
    const size_t off_htmp = hl.add(std::max(sort64_bytes, std::max(sort32_bytes, sort_owner_bytes)));
    Scratch hs(hl, s, who);
    uint32_t *idx = hs.at<uint32_t>(off_idx), *owner = hs.at<uint32_t>(off_owner), *k32a = hs.at<uint32_t>(off_k32a), *k32b = hs.at<uint32_t>(off_k32b);
    uint32_t *sa = hs.at<uint32_t>(off_sa), *sb = hs.at<uint32_t>(off_sb);
    uint64_t *k64a = hs.at<uint64_t>(off_k64a), *k64b = hs.at<uint64_t>(off_k64b);
    unsigned long long* key = hs.at<unsigned long long>(off_key);
    void* htmp = hs.at<void>(off_htmp);
    if (!pstk::radius_long_compact(offsets, long_list, long_offset, n_long, (uint32_t)L, d_indices, d2_keys, idx, k32a, key, owner, s))
      throw hip_failure(who_s + ": compaction launch failed: ");
    // by index; stably by d2 key; stably by the list's place among the long lists
    bytes = sort32_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u32(htmp, bytes, k32a, k32b, sa, sb, L, 32, s, true));
    if (!pstk::radius_gather_u64(key, sb, (uint32_t)L, (unsigned long long*)k64a, s)) throw hip_failure(who_s + ": key gather launch failed: ");
    bytes = sort64_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u64(htmp, bytes, k64a, k64b, sb, sa, L, 64, s));
    if (!pstk::radius_gather_u32(owner, sa, (uint32_t)L, k32a, s)) throw hip_failure(who_s + ": owner gather launch failed: ");
    bytes = sort_owner_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u32(htmp, bytes, k32a, k32b, sa, sb, L, owner_bits, s));
    if (!pstk::radius_long_scatter(offsets, long_list, long_offset, (uint32_t)L, sb, k32b, idx, key, d_indices, d_distances, s))
      throw hip_failure(who_s + ": scatter launch failed: ");
    events.mark(4, s);
    stream_sync(s);  // (the third block of scratch is released behind the scatter)
    events.read();
    return;
  }
  events.mark(4, s);
  stream_sync(s);
  events.read();
}

}  // namespace

extern "C" {

int pst_radius_kernel_shape(uint32_t* queries_per_block, uint32_t* sort_cap_out, uint32_t* sort_window, uint32_t* sort_positions_per_block) {
  if (queries_per_block) *queries_per_block = pstk::kRadiusQueriesPerBlock;
  if (sort_cap_out) *sort_cap_out = pstk::kRadiusSortCap;
  if (sort_window) *sort_window = pstk::kRadiusSortWindow;
  if (sort_positions_per_block) *sort_positions_per_block = pstk::kRadiusSortPositionsPerBlock;
  return PST_OK;
}

int pst_radius_phase_times(double ms[4]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_radius_neighbour_counts_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double radius, uint32_t* d_counts, uint64_t* total) {
  PST_API_BEGIN
  const std::string who = "pst_radius_neighbour_counts_device";
  not_null(index, "index");
  not_null(query, "query");
  if (!d_counts && !total) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": d_counts and total must not both be NULL");
  const Checked c = checked(*query, transform12, radius, who);
  ensure_device();
  check_point_count(query->len, who);
  search(*index, positions_of(*query, *c.pm), c, radius, d_counts, nullptr, false, nullptr, nullptr, 0, total, current_stream(), who);
  PST_API_END
}

int pst_radius_search_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double radius, uint64_t* d_offsets, uint32_t* d_indices,
                             double* d_distances, uint64_t capacity, uint64_t* total) {
  PST_API_BEGIN
  const std::string who = "pst_radius_search_device";
  not_null(index, "index");
  not_null(query, "query");
  not_null(d_offsets, "d_offsets");
  not_null(total, "total");
  if (!d_indices && capacity != 0) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": d_indices may be NULL only with capacity 0 (the counting form)");
  const Checked c = checked(*query, transform12, radius, who);
  ensure_device();
  check_point_count(query->len, who);
  search(*index, positions_of(*query, *c.pm), c, radius, nullptr, d_offsets, true, d_indices, d_distances, capacity, total, current_stream(), who);
  PST_API_END
}

}  // extern "C"
