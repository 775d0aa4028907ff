// Test-only C forwarders to the sorts and scans of pasture_amd/csrc/device_sort.hpp (tests/sort_hooks.py loads them with ctypes;
// tests/test_device_sort.py is the user).  No kernels, no logic: every function hands its arguments on.  Built by pasture_amd/csrc/Makefile
// into pasture_amd/csrc/build/libpst_sort_hooks.so, linked against libpasture_amd.so; none of these names is part of the product's C ABI.
#include "device_sort.hpp"

extern "C" {

int sorthook_radix_sort_pairs_u32(void* tmp, size_t* bytes, uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, size_t n,
                                  unsigned end_bit, void* stream, int iota, int first_hist_ready) {
  return (int)pstk::radix_sort_pairs_u32(tmp, *bytes, keys_a, keys_b, vals_a, vals_b, n, end_bit, (hipStream_t)stream, iota != 0, first_hist_ready != 0);
}

int sorthook_radix_sort_pairs_u64(void* tmp, size_t* bytes, uint64_t* keys_a, uint64_t* keys_b, uint32_t* vals_a, uint32_t* vals_b, size_t n,
                                  unsigned end_bit, void* stream) {
  return (int)pstk::radix_sort_pairs_u64(tmp, *bytes, keys_a, keys_b, vals_a, vals_b, n, end_bit, (hipStream_t)stream);
}

int sorthook_sort_pairs_u32(void* tmp, size_t* bytes, uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n,
                            unsigned end_bit, void* stream, int iota) {
  return (int)pstk::sort_pairs_u32(tmp, *bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, (hipStream_t)stream, iota != 0, nullptr);
}

int sorthook_sort_pairs_u64(void* tmp, size_t* bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, size_t n,
                            unsigned end_bit, void* stream) {
  return (int)pstk::sort_pairs_u64(tmp, *bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, (hipStream_t)stream);
}

void sorthook_radix_sort_first_pass(void* tmp, size_t n, unsigned end_bit, void** counts, uint32_t* tiles, uint32_t* bits, uint32_t* tile_size) {
  const pstk::RadixFirstPass f = pstk::radix_sort_first_pass(tmp, n, end_bit);
  *counts = f.counts;
  *tiles = f.tiles;
  *bits = f.bits;
  *tile_size = f.tile_size;
}

int sorthook_radix_sort_pairs_supported(size_t n, unsigned end_bit) { return pstk::radix_sort_pairs_supported(n, end_bit) ? 1 : 0; }

int sorthook_exclusive_sum_u32_u64(void* tmp, size_t* bytes, const uint32_t* in, unsigned long long* out, size_t n, void* stream) {
  return (int)pstk::exclusive_sum_u32_u64(tmp, *bytes, in, out, n, (hipStream_t)stream);
}

int sorthook_suffix_min_u32(void* tmp, size_t* bytes, uint32_t* data, size_t n, void* stream) {
  return (int)pstk::suffix_min_u32(tmp, *bytes, data, n, (hipStream_t)stream);
}

}  // extern "C"
