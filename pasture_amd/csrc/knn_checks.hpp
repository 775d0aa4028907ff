// The checks of pst_compute_normals_device and its search with only the neighbour lists requested, shared by the entry points that run the kNN
// search for the lists alone (outliers_api.cpp, features_api.cpp).
#pragma once
#include "runtime.hpp"

namespace pst {

// The checks in two halves: what the arguments and the layout alone decide is answered before a device is looked for, the cloud's length
// after it (so a call without a device is PST_ERR_NO_DEVICE whatever the buffer holds).
inline const Member& knn_checked_arguments(const pst_buffer& b, size_t k, const char* who) {
  if (k < 3) throw Error(PST_ERR_K_TOO_SMALL, "The k nearest neigbors attribute is too small!");
  if (k > 64) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": k > 64 is not supported by the register-resident k-best list");
  return position_member(b);
}
inline void knn_checked_length(const pst_buffer& b, size_t at_least, const char* who) {
  if (b.len < 3) throw Error(PST_ERR_TOO_FEW_POINTS, "The point cloud is too small. Please use a point cloud that has 3 or more points!");
  if (b.len < at_least) throw Error(PST_ERR_TOO_FEW_POINTS, std::string(who) + ": the point cloud needs at least " + std::to_string(at_least) + " points");
  check_point_count(b.len, who);
}

// the neighbour lists only; degenerate plane fits (a positive return) are no error here: the lists are written whatever the fit says
inline void knn_lists(const pstk::Positions& pv, size_t k, uint32_t* d_knn, hipStream_t s, const char* who) {
  const long long rc = pstk::run_normals(pv.base, pv.stride, pv.n, (uint32_t)k, nullptr, nullptr, nullptr, d_knn, 0, 0, 0, 0, s);
  if (rc == -2) throw Error(PST_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 17 points per call");
  if (rc < 0) throw hip_failure(std::string(who) + ": neighbour search failed: ");
}

}  // namespace pst
