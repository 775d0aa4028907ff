// pst_knn_search_device / pst_statistical_outlier_mask / pst_radius_outlier_mask: argument checks and plumbing between the kNN search
// (pstk::run_normals with only the uint32 neighbour lists requested, as pst_compute_normals_device calls it) and outliers.hip.
#include <cmath>

#include "device_sort.hpp"
#include "knn_checks.hpp"

using namespace pst;

namespace {

void check_mask_args(const uint8_t* mask, uint32_t mask_memkind, const uint64_t* kept) {
  not_null(mask, "mask");
  not_null(kept, "kept");
  if (mask_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid mask memory kind");
}

struct HostRecord { double stats[4]; unsigned long long kept; };

}  // namespace

extern "C" {

int pst_outlier_kernel_shape(uint32_t* points_per_block, uint32_t* reduce_block, uint32_t* reduce_points_per_block) {
  if (points_per_block) *points_per_block = pstk::kOutlierPointsPerBlock;
  if (reduce_block) *reduce_block = pstk::kOutlierReduceBlock;
  if (reduce_points_per_block) *reduce_points_per_block = pstk::kOutlierReducePoints;
  return PST_OK;
}

int pst_knn_search_device(const pst_buffer* b, size_t k, uint32_t* d_knn, double* d_dist) {
  PST_API_BEGIN
  const char* who = "pst_knn_search_device";
  not_null(b, "buffer");
  not_null(d_dist, "d_dist");
  const Member& pm = knn_checked_arguments(*b, k, who);
  ensure_device();
  knn_checked_length(*b, 3, who);
  hipStream_t s = current_stream();
  const pstk::Positions pv = positions_of(*b, pm);
  Scratch own;
  if (!d_knn) d_knn = own.alloc<uint32_t>(pv.n * k * sizeof(uint32_t), s, who);
  knn_lists(pv, k, d_knn, s, who);
  if (!pstk::outlier_distances(pv, (uint32_t)k, d_knn, d_dist, s)) throw hip_failure("knn_search: distance launch failed: ");
  stream_sync(s);
  PST_API_END
}

int pst_statistical_outlier_mask(const pst_buffer* b, size_t mean_k, double stddev_mult, uint8_t* mask, uint32_t mask_memkind, double* d_mean_dist, double stats[4],
                                 uint64_t* kept) {
  PST_API_BEGIN
  const char* who = "pst_statistical_outlier_mask";
  not_null(b, "buffer");
  check_mask_args(mask, mask_memkind, kept);
  not_null(stats, "stats");
  if (mean_k < 1 || mean_k > 63) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": mean_k must be between 1 and 63");
  if (std::isnan(stddev_mult)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": stddev_mult is NaN");
  const size_t k = std::max<size_t>(mean_k + 1, 3);
  const Member& pm = knn_checked_arguments(*b, k, who);
  ensure_device();
  knn_checked_length(*b, mean_k + 1, who);
  hipStream_t s = current_stream();
  const pstk::Positions pv = positions_of(*b, pm);
  const size_t n = pv.n;
  const bool mask_on_device = mask_memkind == PST_MEM_DEVICE;
  // one block of scratch: neighbour lists | dbar (unless the caller takes it) | block partials | result record | mask (host masks)
  ScratchLayout layout;
  const size_t off_knn = layout.add(n * k * sizeof(uint32_t)), off_dbar = layout.add(d_mean_dist ? 0 : n * sizeof(double));
  const size_t off_part = layout.add(pstk::outlier_partials_bytes(n)), off_rec = layout.add(pstk::outlier_record_bytes());
  const size_t off_mask = layout.add(mask_on_device ? 0 : n);
  Scratch scratch(layout, s, who);
  uint32_t* d_knn = scratch.at<uint32_t>(off_knn);
  double* dbar = d_mean_dist ? d_mean_dist : scratch.at<double>(off_dbar);
  void* rec = scratch.at<void>(off_rec);
  uint8_t* mask_dev = mask_on_device ? mask : scratch.at<uint8_t>(off_mask);
  knn_lists(pv, k, d_knn, s, who);
  if (!pstk::outlier_mean_distances(pv, (uint32_t)k, (uint32_t)mean_k, d_knn, dbar, s) ||
      !pstk::outlier_statistics_and_mask(dbar, n, stddev_mult, scratch.at<void>(off_part), rec, mask_dev, s))
    throw hip_failure("statistical outlier launch failed: ");
  HostRecord r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  if (!mask_on_device) PST_HIP_CHECK(hipMemcpyAsync(mask, mask_dev, n, hipMemcpyDeviceToHost, s));
  stream_sync(s);
  for (int i = 0; i < 4; ++i) stats[i] = r.stats[i];
  *kept = r.kept;
  PST_API_END
}

int pst_radius_outlier_mask(const pst_buffer* b, double radius, size_t min_neighbours, uint8_t* mask, uint32_t mask_memkind, uint64_t* kept) {
  PST_API_BEGIN
  const char* who = "pst_radius_outlier_mask";
  not_null(b, "buffer");
  check_mask_args(mask, mask_memkind, kept);
  if (min_neighbours < 1 || min_neighbours > 63) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": min_neighbours must be between 1 and 63");
  if (!(radius >= 0.0) || std::isinf(radius)) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": radius must be finite and not negative");
  const size_t k = std::max<size_t>(min_neighbours + 1, 3);
  const Member& pm = knn_checked_arguments(*b, k, who);
  ensure_device();
  knn_checked_length(*b, 3, who);
  hipStream_t s = current_stream();
  const pstk::Positions pv = positions_of(*b, pm);
  const size_t n = pv.n;
  const bool mask_on_device = mask_memkind == PST_MEM_DEVICE;
  ScratchLayout layout;  // neighbour lists | result record | mask (host masks)
  const size_t off_knn = layout.add(n * k * sizeof(uint32_t)), off_rec = layout.add(pstk::outlier_record_bytes()), off_mask = layout.add(mask_on_device ? 0 : n);
  Scratch scratch(layout, s, who);
  uint32_t* d_knn = scratch.at<uint32_t>(off_knn);
  void* rec = scratch.at<void>(off_rec);
  uint8_t* mask_dev = mask_on_device ? mask : scratch.at<uint8_t>(off_mask);
  knn_lists(pv, k, d_knn, s, who);
  if (!pstk::outlier_radius_mask(pv, (uint32_t)k, (uint32_t)min_neighbours, radius, d_knn, rec, mask_dev, s)) throw hip_failure("radius outlier launch failed: ");
  HostRecord r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, s));
  if (!mask_on_device) PST_HIP_CHECK(hipMemcpyAsync(mask, mask_dev, n, hipMemcpyDeviceToHost, s));
  stream_sync(s);
  *kept = r.kept;
  PST_API_END
}

}  // extern "C"
