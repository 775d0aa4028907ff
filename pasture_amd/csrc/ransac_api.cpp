// pst_ransac_* / pst_*_inliers / pst_*_inlier_mask_device: sampler, argument checks and plumbing for ransac.hip.
// Reference: pasture-algorithms/src/segmentation.rs:47-94 (hypotheses and their redraw loops), :117-370 (ransac_{plane,line}_{serial,par}).
#include <cmath>
#include <cstring>
#include <vector>

#include "device_sort.hpp"
#include "runtime.hpp"

using namespace pst;

namespace {

// The sampler's recipe (include/pasture_amd.h): ONE counter c, starting at 0, feeds every draw of a call and advances by one per draw, redraws
// included; draw = (splitmix64(seed ^ c) * n) >> 64 from the 128-bit product.
void sample_indices(uint64_t seed, uint64_t n, size_t iterations, uint32_t per, uint64_t* out) {
  uint64_t c = 0;
  auto draw = [&]() { return (uint64_t)(((unsigned __int128)splitmix64(seed ^ c++) * n) >> 64); };
  for (size_t it = 0; it < iterations; ++it) {
    const uint64_t r1 = draw();
    uint64_t r2 = draw();
    while (r1 == r2) r2 = draw();  // segmentation.rs:52-54, :85-87
    out[it * per] = r1;
    out[it * per + 1] = r2;
    if (per == 3) {
      uint64_t r3 = draw();
      while (r2 == r3 || r1 == r3) r3 = draw();  // :57-59
      out[it * per + 2] = r3;
    }
  }
}

const Member* position_member(const pst_buffer& b) {
  const Member* m = position_vec3f64(b);
  if (!m) throw Error(PST_ERR_MISSING_ATTRIBUTE, "Attribute Position3D (Vec3f64) not found in PointLayout of buffer");
  return m;
}
pstk::Positions position_view(const pst_buffer& b, const Member* m) {
  if (b.len >= 0xFFFFFFFFull) throw Error(PST_ERR_UNSUPPORTED, "ransac: 2^32 - 1 points and more per call are not supported");
  pstk::Positions p = positions_of(b, *m);
  if (b.len == 0) p.base = nullptr;
  return p;
}

struct FitResult { uint64_t best, ranking; double model[6]; };

// checks shared by *_fit and the seeded entry points, in the order the header documents
pstk::Positions fit_checks(const pst_buffer* b, size_t iterations, bool line) {
  not_null(b, "buffer");
  if (iterations == 0)  // the reference unwraps the max_by of an empty iterator
    throw Error(PST_ERR_INVALID_ARGUMENT, "called `Option::unwrap()` on a `None` value (num_of_iterations is 0)");
  if (iterations > 0xFFFFFFFFull) throw Error(PST_ERR_UNSUPPORTED, "ransac: 2^32 iterations and more are not supported");
  const Member* m = position_member(*b);
  ensure_device();
  const size_t need = line ? 2 : 3;
  if (b->len < need)
    throw Error(PST_ERR_TOO_FEW_POINTS, line ? "buffer needs to include at least 2 points to generate a line model."
                                             : "buffer needs to include at least 3 points to generate a plane model.");
  return position_view(*b, m);
}

FitResult fit(const pstk::Positions& pv, bool line, double thr, const uint64_t* samples, size_t iterations, uint64_t* rankings) {
  const size_t per = line ? 2 : 3;
  for (size_t it = 0; it < iterations; ++it) {
    const uint64_t* s = samples + it * per;
    for (size_t k = 0; k < per; ++k)
      if (s[k] >= pv.n) throw Error(PST_ERR_RANGE, "ransac: sample index " + std::to_string(s[k]) + " out of range for " + std::to_string(pv.n) + " points");
    if (s[0] == s[1] || (per == 3 && (s[0] == s[2] || s[1] == s[2])))
      throw Error(PST_ERR_INVALID_ARGUMENT, "ransac: hypothesis " + std::to_string(it) + " repeats a point index (the reference redraws until they differ)");
  }
  hipStream_t s = current_stream();
  const size_t rec_bytes = pstk::ransac_record_bytes(line);
  // one block of scratch: samples | records | rankings | result record
  ScratchLayout layout;
  const size_t off_samples = layout.add(iterations * per * sizeof(uint64_t)), off_recs = layout.add(iterations * rec_bytes);
  const size_t off_rank = layout.add(iterations * sizeof(uint64_t)), off_out = layout.add(64);
  Scratch scratch(layout, s, "ransac");
  uint64_t* samples_dev = scratch.at<uint64_t>(off_samples);
  unsigned long long* rank = scratch.at<unsigned long long>(off_rank);
  unsigned long long* out = scratch.at<unsigned long long>(off_out);
  PST_HIP_CHECK(hipMemcpyAsync(samples_dev, samples, iterations * per * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  if (!pstk::ransac_fit(line, pv, thr, samples_dev, iterations, scratch.at<void>(off_recs), rank, out, s)) throw hip_failure("ransac launch failed: ");
  FitResult r{};
  PST_HIP_CHECK(hipMemcpyAsync(&r, out, sizeof(r), hipMemcpyDeviceToHost, s));
  if (rankings) PST_HIP_CHECK(hipMemcpyAsync(rankings, rank, iterations * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  return r;
}

int fit_entry(const pst_buffer* b, bool line, double thr, const uint64_t* samples, size_t iterations, double* model, uint64_t* ranking, size_t* best_iteration,
              uint64_t* rankings) {
  PST_API_BEGIN
  not_null(samples, "samples");
  not_null(model, line ? "line" : "plane");
  not_null(ranking, "ranking");
  const pstk::Positions pv = fit_checks(b, iterations, line);
  const FitResult r = fit(pv, line, thr, samples, iterations, rankings);
  std::memcpy(model, r.model, (line ? 6 : 4) * sizeof(double));
  *ranking = r.ranking;
  if (best_iteration) *best_iteration = (size_t)r.best;
  PST_API_END
}

int seeded_entry(const pst_buffer* b, bool line, double thr, size_t iterations, uint64_t seed, double* model, uint64_t* ranking) {
  PST_API_BEGIN
  not_null(model, line ? "line" : "plane");
  not_null(ranking, "ranking");
  const pstk::Positions pv = fit_checks(b, iterations, line);
  const size_t per = line ? 2 : 3;
  std::vector<uint64_t> samples(iterations * per);
  sample_indices(seed, pv.n, iterations, (uint32_t)per, samples.data());
  const FitResult r = fit(pv, line, thr, samples.data(), iterations, nullptr);
  std::memcpy(model, r.model, (line ? 6 : 4) * sizeof(double));
  *ranking = r.ranking;
  PST_API_END
}

int mask_entry(const pst_buffer* b, bool line, const double* model, double thr, uint8_t* device_mask) {
  PST_API_BEGIN
  not_null(b, "buffer");
  not_null(model, line ? "line" : "plane");
  const Member* m = position_member(*b);
  if (b->len == 0) return PST_OK;
  not_null(device_mask, "device_mask");
  ensure_device();
  const pstk::Positions pv = position_view(*b, m);
  hipStream_t s = current_stream();
  Scratch rec;  // released in stream order behind the mask kernel
  if (!pstk::ransac_mask(line, pv, model, thr, rec.alloc(pstk::ransac_record_bytes(line), s, "ransac"), device_mask, s))
    throw hip_failure("ransac mask launch failed: ");
  PST_API_END
}

int inliers_entry(const pst_buffer* b, bool line, const double* model, double thr, uint64_t* indices, size_t capacity, uint64_t* count) {
  PST_API_BEGIN
  not_null(b, "buffer");
  not_null(model, line ? "line" : "plane");
  not_null(count, "count");
  const Member* m = position_member(*b);
  *count = 0;
  if (b->len == 0) return PST_OK;
  ensure_device();
  const pstk::Positions pv = position_view(*b, m);
  hipStream_t s = current_stream();
  const size_t blocks = (pv.n + pstk::kRansacPointsPerBlock - 1) / pstk::kRansacPointsPerBlock;
  // counts[blocks + 1] (the last one zero, so that the scan's last offset is the total) | offsets[blocks + 1] | record | scan scratch
  size_t scan_bytes = 0;
  if (pstk::exclusive_sum_u32_u64(nullptr, scan_bytes, nullptr, nullptr, blocks + 1, s) != hipSuccess) throw hip_failure("ransac: scan sizing failed: ");
  ScratchLayout layout;
  const size_t off_counts = layout.add((blocks + 1) * sizeof(uint32_t)), off_offsets = layout.add((blocks + 1) * sizeof(uint64_t));
  const size_t off_rec = layout.add(256), off_scan = layout.add(scan_bytes);
  Scratch scratch(layout, s, "ransac");
  uint32_t* counts = scratch.at<uint32_t>(off_counts);
  unsigned long long* offsets = scratch.at<unsigned long long>(off_offsets);
  void* rec = scratch.at<void>(off_rec);
  PST_HIP_CHECK(hipMemsetAsync(counts + blocks, 0, sizeof(uint32_t), s));
  if (!pstk::ransac_model_record(line, model, thr, rec, s) || !pstk::ransac_index_pass(line, pv, rec, counts, offsets, nullptr, false, s))
    throw hip_failure("ransac inlier count launch failed: ");
  PST_HIP_CHECK(pstk::exclusive_sum_u32_u64(scratch.at<void>(off_scan), scan_bytes, counts, offsets, blocks + 1, s));
  unsigned long long total = 0;
  PST_HIP_CHECK(hipMemcpyAsync(&total, offsets + blocks, sizeof(total), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  *count = total;
  if (!indices) return PST_OK;
  if (total > capacity)
    throw Error(PST_ERR_RANGE, "ransac: " + std::to_string(total) + " inliers do not fit the index array of " + std::to_string(capacity));
  if (total == 0) return PST_OK;
  Scratch out;
  unsigned long long* idx_dev = out.alloc<unsigned long long>((size_t)total * sizeof(uint64_t), s, "ransac");
  if (!pstk::ransac_index_pass(line, pv, rec, counts, offsets, idx_dev, true, s)) throw hip_failure("ransac inlier index launch failed: ");
  PST_HIP_CHECK(hipMemcpyAsync(indices, idx_dev, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  PST_API_END
}

}  // namespace

extern "C" {

int pst_ransac_sample_indices(uint64_t seed, size_t n_points, size_t iterations, uint32_t per_hypothesis, uint64_t* out_indices) {
  PST_API_BEGIN
  if (per_hypothesis != 2 && per_hypothesis != 3) throw Error(PST_ERR_INVALID_ARGUMENT, "per_hypothesis must be 3 (plane) or 2 (line)");
  if (n_points < per_hypothesis)  // the redraw loops would never end
    throw Error(PST_ERR_TOO_FEW_POINTS, "buffer needs to include at least " + std::to_string(per_hypothesis) + " points to generate a model.");
  if (iterations == 0) return PST_OK;
  not_null(out_indices, "out_indices");
  sample_indices(seed, n_points, iterations, per_hypothesis, out_indices);
  PST_API_END
}

int pst_ransac_kernel_shape(uint32_t* points_per_wave, uint32_t* points_per_block, uint32_t* blocks_per_cu, uint32_t* batch) {
  if (points_per_wave) *points_per_wave = pstk::kRansacPointsPerWave;
  if (points_per_block) *points_per_block = pstk::kRansacPointsPerBlock;
  if (blocks_per_cu) *blocks_per_cu = pstk::kRansacBlocksPerCu;
  if (batch) *batch = pstk::kRansacBatch;
  return PST_OK;
}

int pst_ransac_plane_fit(const pst_buffer* b, double distance_threshold, const uint64_t* samples, size_t iterations, double plane[4], uint64_t* ranking,
                         size_t* best_iteration, uint64_t* rankings) {
  return fit_entry(b, false, distance_threshold, samples, iterations, plane, ranking, best_iteration, rankings);
}
int pst_ransac_line_fit(const pst_buffer* b, double distance_threshold, const uint64_t* samples, size_t iterations, double line[6], uint64_t* ranking,
                        size_t* best_iteration, uint64_t* rankings) {
  return fit_entry(b, true, distance_threshold, samples, iterations, line, ranking, best_iteration, rankings);
}
int pst_ransac_plane(const pst_buffer* b, double distance_threshold, size_t iterations, uint64_t seed, double plane[4], uint64_t* ranking) {
  return seeded_entry(b, false, distance_threshold, iterations, seed, plane, ranking);
}
int pst_ransac_line(const pst_buffer* b, double distance_threshold, size_t iterations, uint64_t seed, double line[6], uint64_t* ranking) {
  return seeded_entry(b, true, distance_threshold, iterations, seed, line, ranking);
}
int pst_plane_inliers(const pst_buffer* b, const double plane[4], double distance_threshold, uint64_t* indices, size_t capacity, uint64_t* count) {
  return inliers_entry(b, false, plane, distance_threshold, indices, capacity, count);
}
int pst_line_inliers(const pst_buffer* b, const double line[6], double distance_threshold, uint64_t* indices, size_t capacity, uint64_t* count) {
  return inliers_entry(b, true, line, distance_threshold, indices, capacity, count);
}
int pst_plane_inlier_mask_device(const pst_buffer* b, const double plane[4], double distance_threshold, uint8_t* device_mask) {
  return mask_entry(b, false, plane, distance_threshold, device_mask);
}
int pst_line_inlier_mask_device(const pst_buffer* b, const double line[6], double distance_threshold, uint8_t* device_mask) {
  return mask_entry(b, true, line, distance_threshold, device_mask);
}

}  // extern "C"
