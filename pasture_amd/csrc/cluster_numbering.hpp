// The numbering of components, shared by the drivers that label points through a union-find (clusters_api.cpp, dbscan_api.cpp, region_api.cpp):
// everything between "every point has its root, every root its size and its smallest member" and the caller's own label kernel, then the copies
// to the caller's outputs.  The kernels are those of clusters.hip ("flatten and numbering"); the tally in front is grid_index_device.hpp's.
//
//   number_kept    memset flags -> cluster_flag_kept (size filter, the smallest member of every kept component flagged) -> exclusive_sum_u32_u64
//                  (= the kept roots in ascending smallest-member order) -> cluster_list_kept -> the kept count and the call's two counters read
//                  back behind ONE synchronisation -> one STABLE sort_pairs_u32 on 0xFFFFFFFF - size (descending size, ties keep the list's
//                  order) -> cluster_ranks (rank_of_root all ones, then the rank of every kept root; the kept sizes)
//   (the caller's label kernel, which reads rank_of_root, and its last phase mark)
//   finish_numbered  sizes when they fit, labels and byte mask for host outputs, the final synchronisation, events.read(), the counts,
//                  PST_ERR_RANGE when the sizes did not fit
//
// The arrays come by pointer: each caller keeps its own map of which dead region holds which (the comments in the three API files).
#pragma once
#include "device_sort.hpp"
#include "phase_events.hpp"
#include "runtime.hpp"

namespace pst {

// n_ids ids (sorted positions or buffer indices) carry roots; flags and offsets have n + 1 elements, n the buffer's points (min_index names them)
struct NumberingArrays {
  const uint32_t *root, *size, *min_index;
  uint32_t *flags, *root_at, *list_keys, *list_roots, *sorted_keys, *sorted_roots, *rank_of_root;
  unsigned long long* offsets;   // the scan; then the kept sizes
  unsigned long long* counters;  // two on the device, zeroed by the caller: [0] the caller's own, [1] += the kept sizes
  void* tmp;                     // what the 32-bit sort of n pairs and the scan of n + 1 flags ask for
  size_t tmp_bytes;
};

struct Numbered {
  unsigned long long kept, counted[2];
  const unsigned long long* sizes_dev;  // kept sizes, descending
};

inline Numbered number_kept(const NumberingArrays& a, uint64_t n, uint32_t n_ids, uint64_t min_size, uint64_t max_size, hipStream_t s, const std::string& who) {
  if (!pstk::cluster_flag_kept(a.root, a.size, a.min_index, n, n_ids, min_size, max_size, a.flags, a.root_at, a.counters + 1, s)) throw hip_failure(who + ": flag launch failed: ");
  size_t bytes = a.tmp_bytes;
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(a.tmp, bytes, a.flags, a.offsets, n + 1, s));
  if (!pstk::cluster_list_kept(a.flags, a.offsets, a.root_at, a.size, n, a.list_keys, a.list_roots, s)) throw hip_failure(who + ": list launch failed: ");
  Numbered r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r.kept, a.offsets + n, sizeof(r.kept), hipMemcpyDeviceToHost, s));
  PST_HIP_CHECK(hipMemcpyAsync(r.counted, a.counters, sizeof(r.counted), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  bytes = a.tmp_bytes;
  PST_HIP_CHECK(pstk::sort_pairs_u32(a.tmp, bytes, a.list_keys, a.sorted_keys, a.list_roots, a.sorted_roots, (size_t)r.kept, 32, s));  // (nothing kept: no launch)
  r.sizes_dev = a.offsets;  // (the scan's result has been used up)
  if (!pstk::cluster_ranks(a.sorted_keys, a.sorted_roots, (uint32_t)r.kept, n_ids, a.rank_of_root, a.offsets, s)) throw hip_failure(who + ": rank launch failed: ");
  return r;
}

// where a call's results go: labels_dev == labels when they are in device memory already (on_device), the byte mask and the sizes are nullable
struct NumberedOutputs {
  bool on_device;
  uint32_t* labels;
  const uint32_t* labels_dev;
  uint8_t* mask;
  const uint8_t* mask_dev;
  uint64_t* sizes;
  size_t sizes_capacity;
  uint64_t *n_kept, *n_first, *n_labelled;  // n_first (counted[0]) is nullable
};

// `what`: "clusters" or "regions", for the message
template <int N>
inline void finish_numbered(const Numbered& r, const NumberedOutputs& o, size_t n, PhaseEvents<N>& events, hipStream_t s, const std::string& who, const char* what) {
  const bool sizes_fit = r.kept <= o.sizes_capacity;
  if (o.sizes && sizes_fit && r.kept) PST_HIP_CHECK(hipMemcpyAsync(o.sizes, r.sizes_dev, (size_t)r.kept * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (!o.on_device) {
    PST_HIP_CHECK(hipMemcpyAsync(o.labels, o.labels_dev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (o.mask) PST_HIP_CHECK(hipMemcpyAsync(o.mask, o.mask_dev, n, hipMemcpyDeviceToHost, s));
  }
  stream_sync(s);
  events.read();
  *o.n_kept = r.kept;
  if (o.n_first) *o.n_first = r.counted[0];
  *o.n_labelled = r.counted[1];
  if (o.sizes && !sizes_fit)
    throw Error(PST_ERR_RANGE, who + ": " + std::to_string(r.kept) + " " + what + " do not fit the size array of " + std::to_string(o.sizes_capacity));
}

}  // namespace pst
