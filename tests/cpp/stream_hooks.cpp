// Test-only C forwarders to the fused Vec3f64 stream and the AABB record fold, pasture_amd/csrc/stream.hip (tests/stream_hooks.py loads them with
// ctypes; tests/test_stream_seams.py is the user).  No kernels, no logic: every function hands its arguments on.  Built by pasture_amd/csrc/Makefile
// into pasture_amd/csrc/build/libpst_stream_hooks.so, linked against libpasture_amd.so; none of these names is part of the product's C ABI.
//
// kernels.hpp is written for hipcc's translation units; the functions used here are declared again instead -- same signatures: a mismatch is an
// unresolved symbol and fails the link (-z defs), it is never a wrong call.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pstk {
size_t stream_partials_bytes(uint64_t n_points, unsigned mode);
void launch_vec3f64_stream(const double* src, double* dst, uint64_t n_points, const double scale[3], const double offset[3], unsigned mode,
                           double* partials, double* out6, hipStream_t stream);
size_t bounds_partials_bytes(unsigned n_records);
struct ZeroScan { uint64_t base, stride, n; };
void launch_finalize_bounds(double* partials, unsigned n_records, double* out6, hipStream_t stream, const ZeroScan& folded);
void set_bounds_record_form(const void* device_rec6, int form);
}  // namespace pstk

extern "C" {

size_t streamhook_partials_bytes(uint64_t n_points, unsigned mode) { return pstk::stream_partials_bytes(n_points, mode); }

// scale3 / offset3: host arrays of three doubles, or null (identity)
void streamhook_launch(const double* src, double* dst, uint64_t n_points, const double* scale3, const double* offset3, unsigned mode, double* partials,
                       double* out6, void* stream) {
  pstk::launch_vec3f64_stream(src, dst, n_points, scale3, offset3, mode, partials, out6, (hipStream_t)stream);
}

size_t streamhook_bounds_partials_bytes(unsigned n_records) { return pstk::bounds_partials_bytes(n_records); }

void streamhook_finalize_bounds(double* partials, unsigned n_records, double* out6, void* stream, uint64_t zero_base, uint64_t zero_stride,
                                uint64_t zero_n) {
  pstk::launch_finalize_bounds(partials, n_records, out6, (hipStream_t)stream, pstk::ZeroScan{zero_base, zero_stride, zero_n});
}

void streamhook_set_record_form(const void* rec, int form) { pstk::set_bounds_record_form(rec, form); }

}  // extern "C"
