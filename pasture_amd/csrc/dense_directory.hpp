// The host side of the dense directory, shared by the drivers that group entries by a 32-bit key -- a cell of a 2-D grid or a label
// (hag_api.cpp, trees_api.cpp, raster_api.cpp, segments_api.cpp, quantiles_api.cpp).
//
// "The dense directory" over `count` entries in `groups` groups: the caller's keys -> the stable 32-bit pair sort with the entry number as
// payload, which puts the members in group order -- and, within a group, in entry order -- in front of the others -> directory_heads ->
// suffix_min_u32.  Afterwards keys_b holds the sorted keys and `order` the sorted entries, dir[g] is the first sorted position whose group is
// g or later and dir[groups] the number of members: group g is the sorted positions dir[g] .. dir[g + 1].  The kernels that walk it over a
// HagGrid share their device code in dense_grid_device.hpp.
#pragma once
#include <algorithm>

#include "device_sort.hpp"
#include "runtime.hpp"

namespace pst {

// How a key names its group (pstk::directory_heads): `bits` key bits are sorted, the highest of them set in the key of no member.
struct DirectoryKeys { unsigned bits; uint32_t bx, cols; };
// the key is the group: labels 0 .. groups - 1 or row-major cells, then a power of two not below `groups`
inline DirectoryKeys plain_keys(unsigned bits) { return DirectoryKeys{bits, 0, 1}; }
// (cy << bits[0]) | cx of a HagGrid, and the bit above them
inline DirectoryKeys packed_keys(const pstk::HagGrid& g) { return DirectoryKeys{g.bits[0] + g.bits[1] + 1, g.bits[0], g.dim[0]}; }

// The five regions in a call's one block of scratch: keys_a | keys_b | vals_a, `capacity` words each (a caller that sorts something larger
// through them afterwards asks for more than `count`), order (count words), dir (groups + 1 words).
struct DenseDirectory {
  DirectoryKeys keys{};
  size_t count = 0, groups = 0, off[5] = {}, sort_bytes = 0, scan_bytes = 0;
  uint32_t *keys_a = nullptr, *keys_b = nullptr, *vals_a = nullptr, *order = nullptr, *dir = nullptr;

  void carve(ScratchLayout& layout, const DirectoryKeys& k, size_t n_groups, size_t n_entries, size_t capacity, hipStream_t s) {
    keys = k; groups = n_groups; count = n_entries;
    if (count) PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, count, keys.bits, s, true));
    PST_HIP_CHECK(pstk::suffix_min_u32(nullptr, scan_bytes, nullptr, groups + 1, s));
    const size_t bytes[5] = {capacity * 4, capacity * 4, capacity * 4, count * 4, (groups + 1) * 4};
    for (int i = 0; i < 5; ++i) off[i] = layout.add(bytes[i]);
  }
  // of the region `tmp` that build is given
  size_t tmp_bytes() const { return std::max(sort_bytes, scan_bytes); }
  void bind(Scratch& scratch) {
    keys_a = scratch.at<uint32_t>(off[0]); keys_b = scratch.at<uint32_t>(off[1]); vals_a = scratch.at<uint32_t>(off[2]);
    order = scratch.at<uint32_t>(off[3]); dir = scratch.at<uint32_t>(off[4]);
  }
  // fill_keys(keys_a) launches the caller's key kernel over the `count` entries; gather() runs between the sort and the directory (the
  // callers that know the number of members on the host put theirs there).  heads: the sorted positions the heads kernel looks at -- the
  // members where the caller knows their number, else `count`, and the kernel finds the first entry that is no member.  Nothing to look at:
  // every group is empty, and nothing is launched.
  template <class FillKeys, class Gather>
  void build(size_t heads, void* tmp, hipStream_t s, const char* who, FillKeys fill_keys, Gather gather) {
    PST_HIP_CHECK(hipMemsetAsync(dir, heads ? 0xFF : 0, (groups + 1) * 4, s));
    if (heads == 0) return;
    fill_keys(keys_a);
    size_t bytes = sort_bytes;
    PST_HIP_CHECK(pstk::sort_pairs_u32(tmp, bytes, keys_a, keys_b, vals_a, order, count, keys.bits, s, true));
    gather();
    if (!pstk::directory_heads(keys_b, (uint32_t)heads, keys.bx, keys.cols, (uint32_t)groups, dir, s)) throw hip_failure(std::string(who) + ": directory launch failed: ");
    bytes = scan_bytes;
    PST_HIP_CHECK(pstk::suffix_min_u32(tmp, bytes, dir, groups + 1, s));
  }
  template <class FillKeys>
  void build(void* tmp, hipStream_t s, const char* who, FillKeys fill_keys) { build(count, tmp, s, who, fill_keys, [] {}); }
};

}  // namespace pst
