// Test-only C forwarders to the stream-ordered replay of compute_normals, pasture_amd/csrc/normals.hip (tests/knn_hooks.py loads them with
// ctypes; tests/test_knn_replay.py is the user).  No kernels, no logic: every function hands its arguments on or copies fields out.  Built by
// pasture_amd/csrc/Makefile into pasture_amd/csrc/build/libpst_knn_hooks.so, linked against libpasture_amd.so; none of these names is part of
// the product's C ABI.
//
// KnnPlanRecord, GridParams and TileShape come from normals_host.hpp, which pulls in device code: this file is compiled by hipcc, host side
// only.  kernels.hpp names every other launcher and the plan structures of the converters; the functions used here are declared again instead
// -- same signatures: a mismatch is an unresolved symbol and fails the link (-z defs), it is never a wrong call.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "normals_host.hpp"

namespace pstk {
long long run_normals(const uint8_t* pos_base, uint64_t pos_stride, uint64_t n, uint32_t k, double* out_normals_dev, double* out_curv_dev,
                      long long* out_knn_dev, uint32_t* out_knn_u32_dev, uint64_t normal_attr, uint64_t normal_stride, uint64_t curv_attr,
                      uint64_t curv_stride, hipStream_t stream, KnnPlanRecord* record);
struct KnnPlan;
KnnPlan* knn_plan_create(const KnnPlanRecord& rec, bool packed_source, hipStream_t stream);
void knn_plan_free(KnnPlan* p);
const KnnPlanRecord& knn_plan_record(const KnnPlan* p);
KnnPlanCaps knn_plan_caps(const KnnPlan* p);
bool knn_plan_read_counters(const KnnPlan* p, KnnReplayCounters& out, hipStream_t stream);
bool knn_plan_accepts(const KnnPlan* p, const uint8_t* pos_base, uint64_t pos_stride);
bool run_normals_replay(KnnPlan* p, const uint8_t* pos_base, uint64_t pos_stride, double* out_normals_dev, double* out_curv_dev, uint32_t* out_knn_u32_dev,
                        uint64_t normal_attr, uint64_t normal_stride, uint64_t curv_attr, uint64_t curv_stride, unsigned long long* status2, hipStream_t stream);
}  // namespace pstk

extern "C" {

// read-only facts of a plan (tests/knn_hooks.py: KnnFacts mirrors this field for field)
struct knnhook_facts {
  uint64_t n, nf, cells;
  double org[3], h, rot[9], rot_c[3];
  uint32_t dim[3], rx, rotated;
  uint32_t k, key_bits;
  uint32_t bx, by, bz, threads, cap, tag, fit_seq;
  uint32_t use_list, n_list, n_fb, all_boxes, list_cap, fb_cap, staged;
};
struct knnhook_counters {
  uint64_t n_finite;
  uint32_t fb_count, box_count, open_count[2];
  int32_t error_count;
};

// run_normals with a record: -> what run_normals returns; *record = a heap copy of the record (knnhook_record_free), *why_not = its reason
// when it is not valid (a string literal of the library)
long long knnhook_run_normals(const void* pos_base, uint64_t pos_stride, uint64_t n, uint32_t k, double* normals, double* curvature, uint32_t* knn_u32,
                              uint64_t normal_attr, uint64_t normal_stride, uint64_t curv_attr, uint64_t curv_stride, void* stream, void** record, int* valid,
                              const char** why_not) {
  auto* rec = new pstk::KnnPlanRecord;
  const long long rc = pstk::run_normals((const uint8_t*)pos_base, pos_stride, n, k, normals, curvature, nullptr, knn_u32, normal_attr, normal_stride, curv_attr,
                                         curv_stride, (hipStream_t)stream, rec);
  *record = rec;
  *valid = rec->valid ? 1 : 0;
  *why_not = rec->why_not;
  return rc;
}
void knnhook_record_free(void* record) { delete (pstk::KnnPlanRecord*)record; }

void* knnhook_plan_create(const void* record, int packed_source, void* stream) {
  return pstk::knn_plan_create(*(const pstk::KnnPlanRecord*)record, packed_source != 0, (hipStream_t)stream);
}
void knnhook_plan_free(void* plan) { pstk::knn_plan_free((pstk::KnnPlan*)plan); }
int knnhook_plan_accepts(const void* plan, const void* pos_base, uint64_t pos_stride) {
  return pstk::knn_plan_accepts((const pstk::KnnPlan*)plan, (const uint8_t*)pos_base, pos_stride) ? 1 : 0;
}

int knnhook_replay(void* plan, const void* pos_base, uint64_t pos_stride, double* normals, double* curvature, uint32_t* knn_u32, uint64_t normal_attr,
                   uint64_t normal_stride, uint64_t curv_attr, uint64_t curv_stride, void* status2, void* stream) {
  return pstk::run_normals_replay((pstk::KnnPlan*)plan, (const uint8_t*)pos_base, pos_stride, normals, curvature, knn_u32, normal_attr, normal_stride, curv_attr,
                                  curv_stride, (unsigned long long*)status2, (hipStream_t)stream)
             ? 1
             : 0;
}

void knnhook_plan_facts(const void* plan, knnhook_facts* f) {
  const pstk::KnnPlanRecord& r = pstk::knn_plan_record((const pstk::KnnPlan*)plan);
  const pstk::KnnPlanCaps c = pstk::knn_plan_caps((const pstk::KnnPlan*)plan);
  f->n = r.n; f->nf = r.nf; f->cells = r.cells;
  for (int a = 0; a < 3; ++a) { f->org[a] = r.g.org[a]; f->dim[a] = r.g.dim[a]; f->rot_c[a] = r.g.rot_c[a]; }
  for (int a = 0; a < 9; ++a) f->rot[a] = r.g.rot[a];
  f->h = r.g.h; f->rx = r.g.rx; f->rotated = r.g.rotated;
  f->k = r.k; f->key_bits = r.key_bits;
  f->bx = r.shape.bx; f->by = r.shape.by; f->bz = r.shape.bz; f->threads = r.shape.threads; f->cap = r.shape.cap;
  f->tag = (uint32_t)(unsigned char)r.shape.tag; f->fit_seq = r.shape.fit_seq ? 1 : 0;
  f->use_list = r.use_list ? 1 : 0; f->n_list = r.n_list; f->n_fb = r.n_fb;
  f->all_boxes = c.all_boxes; f->list_cap = c.list_cap; f->fb_cap = c.fb_cap; f->staged = c.staged ? 1 : 0;
}

// the plan's device counters after its latest replay (synchronises the stream)
int knnhook_plan_counters(const void* plan, knnhook_counters* out, void* stream) {
  pstk::KnnReplayCounters c;
  if (!pstk::knn_plan_read_counters((const pstk::KnnPlan*)plan, c, (hipStream_t)stream)) return 0;
  out->n_finite = c.n_finite; out->fb_count = c.fb_count; out->box_count = c.box_count;
  out->open_count[0] = c.open_count[0]; out->open_count[1] = c.open_count[1]; out->error_count = c.error_count;
  return 1;
}

}  // extern "C"
