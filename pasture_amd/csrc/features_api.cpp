// pst_geometric_features_from_knn_device / pst_geometric_features / pst_features_kernel_shape: argument checks and plumbing between the kNN
// search (pstk::run_normals with only the uint32 neighbour lists requested, as pst_knn_search_device calls it) and features.hip.
#include <cmath>

#include "knn_checks.hpp"

using namespace pst;

namespace {

// what both entries ask of their parameters, before a device is looked for
void check_feature_args(double max_distance, uint32_t features, const double* d_out, const double* d_normals, const double* d_directions, const char* who) {
  if (std::isnan(max_distance) || max_distance < 0.0) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_distance must not be negative or NaN (+inf: no limit)");
  if (features == 0 || features > PST_FEATURE_ALL) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": features must be a non-empty set of PST_FEATURE_* bits");
  if (!d_out && !d_normals && !d_directions) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": at least one of d_out, d_normals and d_directions must be given");
}

}  // namespace

extern "C" {

int pst_features_kernel_shape(size_t k, uint32_t* points_per_block, uint32_t* threads) {
  PST_API_BEGIN
  if (k < 1 || k > 64) throw Error(PST_ERR_INVALID_ARGUMENT, "pst_features_kernel_shape: k must be between 1 and 64");
  if (points_per_block) *points_per_block = pstk::features_points_per_block((uint32_t)k);
  if (threads) *threads = pstk::kFeaturesThreads;
  PST_API_END
}

int pst_geometric_features_from_knn_device(const pst_buffer* b, size_t k, const uint32_t* d_knn, double max_distance, uint32_t features, double* d_out,
                                           double* d_normals, double* d_directions) {
  PST_API_BEGIN
  const char* who = "pst_geometric_features_from_knn_device";
  not_null(b, "buffer");
  not_null(d_knn, "d_knn");
  if (k < 1 || k > 64) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": k must be between 1 and 64");
  check_feature_args(max_distance, features, d_out, d_normals, d_directions, who);
  const Member& pm = position_member(*b);
  if (b->len == 0) return PST_OK;
  ensure_device();
  check_point_count(b->len, who);
  if (!pstk::geometric_features(positions_of(*b, pm), (uint32_t)k, d_knn, max_distance, features, d_out, d_normals, d_directions, current_stream()))
    throw hip_failure("geometric features launch failed: ");
  PST_API_END
}

int pst_geometric_features(const pst_buffer* b, size_t k, double max_distance, uint32_t features, double* d_out, double* d_normals, double* d_directions,
                           uint32_t* d_knn) {
  PST_API_BEGIN
  const char* who = "pst_geometric_features";
  not_null(b, "buffer");
  check_feature_args(max_distance, features, d_out, d_normals, d_directions, who);
  const Member& pm = knn_checked_arguments(*b, k, who);
  ensure_device();
  knn_checked_length(*b, 3, who);
  hipStream_t s = current_stream();
  const pstk::Positions pv = positions_of(*b, pm);
  Scratch own;
  if (!d_knn) d_knn = own.alloc<uint32_t>(pv.n * k * sizeof(uint32_t), s, who);
  knn_lists(pv, k, d_knn, s, who);
  if (!pstk::geometric_features(pv, (uint32_t)k, d_knn, max_distance, features, d_out, d_normals, d_directions, s)) throw hip_failure("geometric features launch failed: ");
  stream_sync(s);
  PST_API_END
}

}  // extern "C"
