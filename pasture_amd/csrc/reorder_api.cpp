// pst_buffer_gather / _async / pst_buffer_take, pst_sort_order_by_attribute_device, pst_morton_order_device, pst_shuffle_order_device,
// pst_invert_order_device, pst_reorder_kernel_shape, pst_reorder_phase_times: argument checks, the attribute tables, the scratch and the order
// of the launches of reorder.hip (where the kernels are described; the definitions are in include/pasture_amd.h).
#include <cmath>
#include <cstring>
#include <memory>
#include <utility>

#include "cluster_index.hpp"
#include "phase_events.hpp"

using namespace pst;

namespace {

thread_local double t_phase_ms[3] = {0.0, 0.0, 0.0};  // PST_REORDER_TIMES=1: {bounds + keys, sort, gather} of every synchronous call

bool times_wanted() {
  static const bool wanted = env_nonzero("PST_REORDER_TIMES");
  return wanted;
}

struct TempDev {
  uint8_t* p = nullptr;
  explicit TempDev(size_t bytes) { p = bytes ? dev_alloc(bytes, PST_MEM_DEVICE) : nullptr; }
  ~TempDev() { dev_free(p, PST_MEM_DEVICE); }
};

// the byte ranges a buffer's points occupy
void byte_ranges(const pst_buffer& b, std::vector<std::pair<uint64_t, uint64_t>>& out) {
  if (!b.columnar) {
    if (b.len && b.layout.size) out.emplace_back((uint64_t)(uintptr_t)b.data, (uint64_t)b.len * b.layout.size);
    return;
  }
  for (size_t a = 0; a < b.columns.size(); ++a)
    if (b.len && b.layout.members[a].size) out.emplace_back((uint64_t)(uintptr_t)b.columns[a], (uint64_t)b.len * b.layout.members[a].size);
}
bool overlap(const pst_buffer& x, const pst_buffer& y) {
  std::vector<std::pair<uint64_t, uint64_t>> rx, ry;
  byte_ranges(x, rx);
  byte_ranges(y, ry);
  for (auto& p : rx)
    for (auto& q : ry)
      if (p.first < q.first + q.second && q.first < p.first + p.second) return true;
  return false;
}

// checks 1 .. 5 of the gathers, in the documented order; the device comes after them
void check_gather(const pst_buffer* src, const void* indices, uint32_t index_bits, size_t count, const pst_buffer* dst, size_t dst_first, const std::string& who) {
  not_null(src, "src");
  not_null(dst, "dst");
  if (index_bits != 32 && index_bits != 64) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": index_bits must be 32 or 64");
  if (count) not_null(indices, "indices");
  if (dst->layout != src->layout) throw Error(PST_ERR_LAYOUT_MISMATCH, "PointLayouts must match");
  if (overlap(*src, *dst)) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": src and dst overlap (there is no in-place permutation)");
  if (dst_first > dst->len || count > dst->len - dst_first) throw Error(PST_ERR_RANGE, who + ": dst_first + count exceeds the length of dst");
}

// the launches of one gather, stream-ordered; idx_dev: device memory
void launch_gather(const pst_buffer& src, const void* idx_dev, uint32_t index_bits, size_t count, pst_buffer& dst, size_t dst_first, unsigned long long* skipped_dev,
                   hipStream_t s) {
  const size_t na = src.layout.members.size();
  const uint32_t stride = (uint32_t)src.layout.size;
  const bool src_aos = !src.columnar, dst_aos = !dst.columnar;
  pstk::GatherArgs g{};
  g.idx = idx_dev;
  g.idx64 = index_bits == 64;
  g.count = count;
  g.src_len = src.len;
  g.src_rec = src_aos ? aos_addr(src, 0) : 0;
  g.dst_rec = dst_aos ? aos_addr(dst, dst_first) : 0;
  g.stride = stride;
  g.chunk = pstk::gather_chunk(stride);
  g.skipped = skipped_dev;
  g.count_skipped = 1;
  const bool by_bytes = (src_aos || dst_aos) && !pstk::gather_tile_fits(stride);
  if (src_aos && dst_aos) {  // whole records, padding included
    if (by_bytes) {
      g.n_attrs = 1;
      g.attrs[0] = pstk::GatherAttr{g.src_rec, g.dst_rec, stride, stride, 0, stride};
    }
    if (!pstk::gather_points(g, true, true, by_bytes, s)) throw hip_failure("gather launch failed: ");
    return;
  }
  size_t covered = 0;
  for (const Member& m : src.layout.members) covered += m.size;
  const bool one_launch = na <= (size_t)pstk::kReorderMaxAttrs;
  g.dst_covered = covered == stride && one_launch;
  size_t a0 = 0;
  do {  // (a layout without attributes still counts the skipped entries)
    const size_t a1 = std::min(na, a0 + (size_t)pstk::kReorderMaxAttrs);
    g.n_attrs = (uint32_t)(a1 - a0);
    for (size_t a = a0; a < a1; ++a) {
      const Member& m = src.layout.members[a];
      const AttrView sv = attr_view(src, a), dv = attr_view(dst, a, dst_first);
      g.attrs[a - a0] = pstk::GatherAttr{sv.addr, dv.addr, (uint32_t)sv.stride, (uint32_t)dv.stride, (uint32_t)m.offset, (uint32_t)m.size};
    }
    if (!pstk::gather_points(g, src_aos, dst_aos, by_bytes, s)) throw hip_failure("gather launch failed: ");
    g.count_skipped = 0;
    a0 = a1;
  } while (a0 < na);
}

// Synchronous and validated: the list is checked on the device first, so that a bad one leaves dst untouched.  After check_gather, count > 0.
void gather_checked(const pst_buffer& src, const void* indices, uint32_t index_bits, bool on_device, size_t count, pst_buffer& dst, size_t dst_first, const std::string& who) {
  hipStream_t s = current_stream();
  const size_t idx_bytes = count * (index_bits / 8);
  TempDev staged(on_device ? 0 : idx_bytes);
  const void* idx_dev = indices;
  if (!on_device) {
    PST_HIP_CHECK(hipMemcpyAsync(staged.p, indices, idx_bytes, hipMemcpyHostToDevice, s));
    idx_dev = staged.p;
  }
  TempDev words(2 * sizeof(unsigned long long));
  unsigned long long* check = (unsigned long long*)words.p;
  PST_HIP_CHECK(hipMemsetAsync(check, 0, 2 * sizeof(unsigned long long), s));
  if (!pstk::gather_index_check(idx_dev, index_bits == 64, count, src.len, check, s)) throw hip_failure(who + ": index check launch failed: ");
  unsigned long long seen[2] = {0, 0};
  PST_HIP_CHECK(hipMemcpyAsync(seen, check, sizeof(seen), hipMemcpyDeviceToHost, s));
  stream_sync(s);
  if (seen[1])
    throw Error(PST_ERR_RANGE, who + ": " + std::to_string(seen[1]) + " of the indices are out of range (the largest is " + std::to_string(seen[0]) + ", src has " +
                                   std::to_string(src.len) + " points)");
  PhaseEvents<3> events(times_wanted(), t_phase_ms);  // (a gather has no key and no sort phase: those two read as zero)
  for (int i = 0; i < 3; ++i) events.mark(i, s);
  launch_gather(src, idx_dev, index_bits, count, dst, dst_first, nullptr, s);
  events.mark(3, s);
  stream_sync(s);  // the staged indices are released on return
  events.read();
}

void check_order_length(size_t n, const std::string& who) {
  if (n >= 0xFFFFFFF0ull) throw Error(PST_ERR_UNSUPPORTED, who + ": sort orders of 2^32 - 16 points and more are not supported");
}

// keys (by `fill`) -> stable sort with the element numbers as values -> d_order.  fill(keys32, keys64, vals) leaves vals alone for 32-bit keys.
template <typename Fill>
void sort_order(size_t n, bool keys64, unsigned end_bit, uint32_t* d_order, hipStream_t s, PhaseEvents<3>& events, const std::string& who, Fill&& fill) {
  size_t sort_bytes = 0;
  if (keys64) PST_HIP_CHECK(pstk::sort_pairs_u64(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit, s));
  else PST_HIP_CHECK(pstk::sort_pairs_u32(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit, s, true));
  const size_t kb = n * (keys64 ? 8 : 4);
  ScratchLayout layout;
  const size_t off_a = layout.add(kb), off_b = layout.add(kb), off_v = layout.add(n * 4), off_tmp = layout.add(sort_bytes);
  Scratch scratch(layout, s, who.c_str());
  uint32_t* vals = scratch.at<uint32_t>(off_v);
  if (!fill(scratch.at<uint32_t>(off_a), scratch.at<unsigned long long>(off_a), vals)) throw hip_failure(who + ": key launch failed: ");
  events.mark(1, s);
  size_t bytes = sort_bytes;
  if (keys64) PST_HIP_CHECK(pstk::sort_pairs_u64(scratch.at<void>(off_tmp), bytes, scratch.at<uint64_t>(off_a), scratch.at<uint64_t>(off_b), vals, d_order, n, end_bit, s));
  else PST_HIP_CHECK(pstk::sort_pairs_u32(scratch.at<void>(off_tmp), bytes, scratch.at<uint32_t>(off_a), scratch.at<uint32_t>(off_b), vals, d_order, n, end_bit, s, true));
  events.mark(2, s);
  events.mark(3, s);
  stream_sync(s);
  events.read();
}

}  // namespace

extern "C" {

int pst_reorder_kernel_shape(uint32_t* points_per_block, uint32_t* record_tile_bytes) {
  if (points_per_block) *points_per_block = pstk::kReorderPointsPerBlock;
  if (record_tile_bytes) *record_tile_bytes = pstk::kReorderRecordTileBytes;
  return PST_OK;
}

int pst_reorder_phase_times(double ms[3]) {
  PST_API_BEGIN
  not_null(ms, "ms");
  std::memcpy(ms, t_phase_ms, sizeof(t_phase_ms));
  PST_API_END
}

int pst_buffer_gather(const pst_buffer* src, const void* indices, uint32_t index_bits, uint32_t indices_memkind, size_t count, pst_buffer* dst, size_t dst_first) {
  PST_API_BEGIN
  const std::string who = "pst_buffer_gather";
  if (indices_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid indices memory kind");
  check_gather(src, indices, index_bits, count, dst, dst_first, who);
  if (count == 0) return PST_OK;
  ensure_device();
  gather_checked(*src, indices, index_bits, indices_memkind == PST_MEM_DEVICE, count, *dst, dst_first, who);
  PST_API_END
}

int pst_buffer_gather_async(const pst_buffer* src, const void* device_indices, uint32_t index_bits, size_t count, pst_buffer* dst, size_t dst_first,
                            uint64_t* device_skipped) {
  PST_API_BEGIN
  check_gather(src, device_indices, index_bits, count, dst, dst_first, "pst_buffer_gather_async");
  if (count == 0 && !device_skipped) return PST_OK;
  ensure_device();
  hipStream_t s = current_stream();
  if (device_skipped) PST_HIP_CHECK(hipMemsetAsync(device_skipped, 0, sizeof(uint64_t), s));
  if (count) launch_gather(*src, device_indices, index_bits, count, *dst, dst_first, reinterpret_cast<unsigned long long*>(device_skipped), s);
  PST_API_END
}

int pst_buffer_take(const pst_buffer* src, const void* indices, uint32_t index_bits, uint32_t indices_memkind, size_t count, uint32_t out_storage, pst_buffer** out) {
  PST_API_BEGIN
  const std::string who = "pst_buffer_take";
  not_null(src, "src");
  not_null(out, "out");
  if (index_bits != 32 && index_bits != 64) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": index_bits must be 32 or 64");
  if (indices_memkind > PST_MEM_PINNED_HOST) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid indices memory kind");
  if (out_storage > PST_STORAGE_COLUMNAR) throw Error(PST_ERR_INVALID_ARGUMENT, "invalid storage kind");
  if (count) not_null(indices, "indices");
  auto b = std::make_unique<pst_buffer>();
  b->layout = src->layout;
  b->columnar = out_storage == PST_STORAGE_COLUMNAR;
  if (b->columnar) b->columns.assign(b->layout.members.size(), nullptr);
  if (count) {
    ensure_device();
    resize_buffer(*b, count, false);  // every byte of the attributes is overwritten; padding stays as allocated ...
    size_t covered = 0;
    for (auto& m : b->layout.members) covered += m.size;
    // ... except record padding no gather writes, which VectorBuffer::resize zero-fills (as pst_buffer_filter does)
    if (!b->columnar && src->columnar && covered != b->layout.size) PST_HIP_CHECK(hipMemsetAsync(b->data, 0, count * b->layout.size, current_stream()));
    gather_checked(*src, indices, index_bits, indices_memkind == PST_MEM_DEVICE, count, *b, 0, who);
  }
  *out = b.release();
  PST_API_END
}

int pst_sort_order_by_attribute_device(const pst_buffer* b, const char* name, const pst_datatype* dt, uint32_t component, uint32_t descending, uint32_t* d_order) {
  PST_API_BEGIN
  const std::string who = "pst_sort_order_by_attribute_device";
  not_null(b, "buffer");
  not_null(name, "name");
  not_null(dt, "datatype");
  not_null(d_order, "d_order");
  const DataType type = DataType::from_c(dt);
  if (!(type.is_scalar() || type.is_vec3())) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": only numeric attributes have a sort order (not " + type.display() + ")");
  if (component >= type.num_components()) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": component beyond the datatype");
  const Member& m = required(b->layout.find(AttributeDef{name, type}));
  const size_t n = b->len;
  if (n == 0) return PST_OK;
  ensure_device();
  check_order_length(n, who);
  hipStream_t s = current_stream();
  const uint32_t ct = type.comp_type();
  const uint32_t width = (uint32_t)(type.size() / type.num_components());  // bytes of a component
  const AttrView v = attr_view(*b, &m);
  PhaseEvents<3> events(times_wanted(), t_phase_ms);
  events.mark(0, s);
  sort_order(n, width == 8, 8 * width, d_order, s, events, who, [&](uint32_t* k32, unsigned long long* k64, uint32_t* vals) {
    return pstk::reorder_attribute_keys(v.addr + (uint64_t)component * width, v.stride, n, ct, descending != 0, k32, k64, vals, s);
  });
  PST_API_END
}

int pst_morton_order_device(const pst_buffer* b, uint32_t dims, uint32_t bits, uint32_t* d_order, uint64_t* d_keys) {
  PST_API_BEGIN
  const std::string who = "pst_morton_order_device";
  not_null(b, "buffer");
  not_null(d_order, "d_order");
  if (dims != 2 && dims != 3) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": dims must be 2 or 3");
  const uint32_t max_bits = dims == 2 ? 31 : 21;
  if (bits > max_bits) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": bits per axis must be 1 .. " + std::to_string(max_bits) + " (0: that maximum)");
  if (bits == 0) bits = max_bits;
  const Member& pm = position_member(*b);
  const size_t n = b->len;
  if (n == 0) return PST_OK;
  ensure_device();
  check_order_length(n, who);
  hipStream_t s = current_stream();
  const pstk::Positions pos = positions_of(*b, pm);
  PhaseEvents<3> events(times_wanted(), t_phase_ms);
  events.mark(0, s);
  FiniteBounds r{};
  {
    ScratchLayout layout;
    const size_t off_partials = layout.add(pstk::sample_bounds_partials_bytes(n)), off_rec = layout.add(256);
    Scratch scratch(layout, s, who.c_str());
    r = finite_bounds_folded(pos, scratch.at<void>(off_partials), scratch.at<pstk::SampleBounds>(off_rec), s, who);
  }
  pstk::MortonGrid g{};
  g.dims = dims;
  g.bits = bits;
  const double lim = std::ldexp(1.0, (int)bits);
  for (int a = 0; a < 3; ++a) {
    g.min[a] = r.min[a];
    const double inv = lim / (r.max[a] - r.min[a]);  // (no finite point: never used)
    g.inv[a] = (r.count != 0 && r.max[a] != r.min[a] && std::isfinite(inv)) ? inv : 0.0;
  }
  sort_order(n, true, dims * bits + 1, d_order, s, events, who, [&](uint32_t*, unsigned long long* k64, uint32_t* vals) {
    return pstk::reorder_morton_keys(pos, g, k64, vals, reinterpret_cast<unsigned long long*>(d_keys), s);
  });
  PST_API_END
}

int pst_shuffle_order_device(uint64_t n, uint64_t seed, uint32_t* d_order) {
  PST_API_BEGIN
  const std::string who = "pst_shuffle_order_device";
  if (n == 0) return PST_OK;
  not_null(d_order, "d_order");
  ensure_device();
  check_order_length(n, who);
  hipStream_t s = current_stream();
  PhaseEvents<3> events(times_wanted(), t_phase_ms);
  events.mark(0, s);
  sort_order(n, true, 64, d_order, s, events, who,
             [&](uint32_t*, unsigned long long* k64, uint32_t* vals) { return pstk::reorder_shuffle_keys(n, seed, k64, vals, s); });
  PST_API_END
}

int pst_invert_order_device(const uint32_t* d_order, uint64_t n, uint32_t* d_inverse) {
  PST_API_BEGIN
  const std::string who = "pst_invert_order_device";
  if (n == 0) return PST_OK;
  not_null(d_order, "d_order");
  not_null(d_inverse, "d_inverse");
  if (d_order == d_inverse) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": d_order and d_inverse are the same array (there is no in-place inversion)");
  ensure_device();
  check_order_length(n, who);
  if (!pstk::reorder_invert(d_order, n, d_inverse, current_stream())) throw hip_failure(who + ": launch failed: ");
  PST_API_END
}

}  // extern "C"
