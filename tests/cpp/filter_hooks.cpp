// Test-only C forwarders to the count and scan phase of the compaction, pasture_amd/csrc/filter.hip (tests/filter_hooks.py loads them with ctypes;
// tests/test_filter_seams.py is the user).  No kernels, no logic: every function hands its arguments on.  Built by pasture_amd/csrc/Makefile
// into pasture_amd/csrc/build/libpst_filter_hooks.so, linked against libpasture_amd.so; none of these names is part of the product's C ABI.
//
// kernels.hpp is written for hipcc's translation units (it names std::vector without including it, and pulls in the plan structures and every
// other launcher); the four functions used here are declared again instead -- same signatures: a mismatch is an unresolved symbol and fails the link
// (-z defs), it is never a wrong call.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pstk {
size_t filter_workspace_bytes(uint64_t n);
uint32_t filter_tile(bool dst_aos, uint32_t dst_stride);
void launch_filter_count(const uint8_t* mask_dev, uint64_t n, uint32_t tile, uint8_t* workspace, const unsigned long long** out_total_dev,
                         hipStream_t stream, unsigned long long* total_also);
uint32_t* filter_counts(uint8_t* workspace, uint64_t n, uint32_t tile);
}  // namespace pstk

extern "C" {

size_t filterhook_workspace_bytes(uint64_t n) { return pstk::filter_workspace_bytes(n); }

uint32_t filterhook_tile() { return pstk::filter_tile(false, 0); }

// -> where the launch says the total lies (offsets + n_tiles)
const void* filterhook_count(const uint8_t* mask, uint64_t n, uint32_t tile, uint8_t* workspace, void* stream, unsigned long long* total_also) {
  const unsigned long long* total = nullptr;
  pstk::launch_filter_count(mask, n, tile, workspace, &total, (hipStream_t)stream, total_also);
  return total;
}

void filterhook_layout(uint8_t* workspace, uint64_t n, uint32_t tile, void** offsets, void** counts) {
  *offsets = workspace;
  *counts = pstk::filter_counts(workspace, n, tile);
}

}  // extern "C"
