// Internal host runtime declarations: device buffers, per-thread workspace, plan execution.
#pragma once
#include <cmath>
#include <cstdlib>
#include <atomic>
#include <memory>
#include <vector>

#include "core.hpp"
#include "device_sort.hpp"
#include "kernels.hpp"
#include "plan.h"
#include "scratch_layout.hpp"

// Device-backed point buffer.  One struct serves the three reference buffer kinds:
//   VectorBuffer          (point_buffer.rs:659-945)   columnar = false, owns = true
//   HashMapBuffer         (point_buffer.rs:1031-1474) columnar = true,  owns = true   (one 256-B aligned column per attribute;
//                          the per-point HashMap lookup of :1222-1235 becomes a pointer table indexed by layout slot)
//   ExternalMemoryBuffer  (point_buffer.rs:1479-1708) owns = false (caller's device memory)
struct pst_buffer {
  pst::Layout layout;
  bool columnar = false;
  bool owns = true;
  uint32_t memkind = PST_MEM_DEVICE;
  size_t len = 0;       // points
  size_t capacity = 0;  // points
  uint8_t* data = nullptr;         // interleaved storage
  std::vector<uint8_t*> columns;   // columnar storage, layout order
  // Slices borrow the parent's storage (slice.rs:16-43; Rust's borrow checker keeps the parent untouched while one lives).  The C ABI has no
  // borrow checker, so an owning buffer carries a storage epoch -- bumped whenever its storage moves, shrinks, grows or dies -- and a slice
  // remembers the epoch it was cut at: any use of a slice whose parent has been resized or destroyed since is PST_ERR_INVALID_ARGUMENT
  // instead of a read of freed device memory.
  // owning buffers: their own, made WITH the buffer (cutting a slice only reads the parent: two threads may slice one buffer at once); slices: the owning
  // ancestor's; external memory: none
  std::shared_ptr<std::atomic<uint64_t>> epoch = std::make_shared<std::atomic<uint64_t>>(0);
  uint64_t epoch_cut = 0;                        // slices: the ancestor's epoch when the slice was cut
  bool is_slice = false;
  ~pst_buffer();
};

namespace pst {

// per-thread scratch: device partials / result records + a pinned host mirror for small read-backs
struct Workspace {
  uint8_t* dev = nullptr;     // kWorkspaceBytes: small result records
  uint8_t* pinned = nullptr;  // kPinnedBytes
  uint8_t* partials_buf = nullptr;  // grow-only scratch for per-block reduction records
  size_t partials_cap = 0;
  static constexpr size_t kWorkspaceBytes = 1u << 20;
  static constexpr size_t kPinnedBytes = 1u << 12;
  // device scratch of at least `bytes` (grows by reallocation; growth synchronises the device once)
  uint8_t* partials(size_t bytes);
};
Workspace& workspace();
// Small result records a SYNCHRONOUS entry point waits for (an AABB, the encoder's header contribution) are written by the call's last kernel straight
// into the pinned mirror -- host memory the device addresses -- instead of into device memory and copied out by one more launch (a blit kernel per
// hipMemcpyAsync).  PST_RESULTS_TO_HOST=0: the copy (the A/B switch).
inline bool results_to_host() {
  static const bool on = env_on("PST_RESULTS_TO_HOST");
  return on;
}

uint8_t* dev_alloc(size_t bytes, uint32_t memkind);
void dev_free(uint8_t* p, uint32_t memkind);
// no-throw forms on an explicit stream (stream-ordered pool, or hipMalloc / hipFree without pool support or with PST_NO_POOL)
hipError_t dev_alloc_stream(void** p, size_t bytes, hipStream_t s);  // (out of memory: the pool's unused blocks are given back and the request repeated once)
hipError_t dev_malloc_retry(void** p, size_t bytes);  // hipMalloc with the same second chance
void trim_device_pool();  // pst_release_scratch: unused pool blocks of the current device back to the driver
void dev_free_stream(void* p, hipStream_t s);

// every API entry takes its buffers through not_null(b, "..."): this overload is where a stale slice is caught
void check_live(const pst_buffer& b);
inline const pst_buffer* not_null(const pst_buffer* p, const char* what) {
  if (!p) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(what) + " must not be NULL");
  check_live(*p);
  return p;
}
inline pst_buffer* not_null(pst_buffer* p, const char* what) {
  if (!p) throw Error(PST_ERR_INVALID_ARGUMENT, std::string(what) + " must not be NULL");
  check_live(*p);
  return p;
}
void bump_epoch(pst_buffer& b);  // the storage of an owning buffer is about to move or die

// address helpers
inline uint64_t aos_addr(const pst_buffer& b, size_t point) { return (uint64_t)(uintptr_t)b.data + (uint64_t)point * b.layout.size; }
inline uint64_t col_addr(const pst_buffer& b, size_t slot, size_t point) {
  return (uint64_t)(uintptr_t)b.columns[slot] + (uint64_t)point * b.layout.members[slot].size;
}
// where the values of one attribute are: the address of point `first`'s value and the distance in bytes to the next point's
struct AttrView { uint64_t addr; uint64_t stride; };
inline AttrView attr_view(const pst_buffer& b, size_t slot, size_t first = 0) {
  const Member& m = b.layout.members[slot];
  return b.columnar ? AttrView{col_addr(b, slot, first), m.size} : AttrView{aos_addr(b, first) + m.offset, b.layout.size};
}
// m: a member of b's own layout, or null for an attribute the layout does not have => {0, 0}
inline AttrView attr_view(const pst_buffer& b, const Member* m, size_t first = 0) {
  return m ? attr_view(b, (size_t)(m - b.layout.members.data()), first) : AttrView{0, 0};
}
// the positions as the launchers take them; m: the buffer's Position3D member (position_vec3f64).  No checks: the length limits are the callers'
inline pstk::Positions positions_of(const pst_buffer& b, const Member& m) {
  const AttrView v = attr_view(b, &m);
  return pstk::Positions{(const uint8_t*)(uintptr_t)v.addr, v.stride, b.len};
}
// view_attribute::<Vector3<f64>>(&POSITION_3D): exact name AND datatype (buffer_views.rs:301-310); null when the layout has none (each caller
// throws the message of the panic it mirrors)
inline const Member* position_vec3f64(const pst_buffer& b) {
  AttributeDef pos{"Position3D", DataType{}};
  pos.datatype.kind = PST_VEC3F64;
  return b.layout.find(pos);
}
// what Layout::find returned, or the panic of view_attribute on a layout without the attribute
inline const Member& required(const Member* m) {
  if (!m) throw Error(PST_ERR_MISSING_ATTRIBUTE, "Attribute not found in PointLayout of buffer");
  return *m;
}
inline const Member& position_member(const pst_buffer& b) { return required(position_vec3f64(b)); }
// the kernels' point indices are uint32_t, and the largest sixteen values are kept free
inline void check_point_count(size_t n, const std::string& who) {
  if (n >= 0xFFFFFFF0ull) throw Error(PST_ERR_UNSUPPORTED, who + ": more than 2^32 - 17 points per call");
}

// max_distance of the neighbour searches (nn_api.cpp, hag_api.cpp), checked; returns m2 = max_distance * max_distance, rounded once
inline double checked_m2(double max_distance, const char* who) {
  const double m2 = max_distance * max_distance;
  if (std::isnan(max_distance) || !(max_distance > 0.0) || !(std::isnormal(m2) || std::isinf(m2)))
    throw Error(PST_ERR_INVALID_ARGUMENT, std::string(who) + ": max_distance must be positive (+inf: unbounded), and its square a normal number or +inf");
  return m2;
}

// the finaliser synth.hip uses for pst_buffer_synth_fill: the draws of the RANSAC sampler (ransac_api.cpp) and the shuffled priority keys of
// the subsampling (sample_api.cpp; sample.hip evaluates the same per candidate)
inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The raster over an AABB in x and y (pmf_api.cpp, raster_api.cpp): dim = cell of the largest coordinate + 1, by the expression the kernels
// evaluate per point
inline pstk::PmfGrid pmf_grid_over(double min_x, double min_y, double max_x, double max_y, double cell, const std::string& who) {
  constexpr uint64_t kMaxCells = 1ull << 28;
  pstk::PmfGrid g{};
  g.x0 = min_x;
  g.y0 = min_y;
  g.cell = cell;
  const double qx = (max_x - g.x0) / cell, qy = (max_y - g.y0) / cell;
  // (a quotient that is not below 2^28 -- an extent that overflows f64 included -- is refused before it is converted)
  const bool fits = qx < (double)kMaxCells && qy < (double)kMaxCells && ((uint64_t)qx + 1) * ((uint64_t)qy + 1) <= kMaxCells;
  if (!fits) throw Error(PST_ERR_UNSUPPORTED, who + ": the raster would have more than 2^28 cells: use a larger cell_size");
  g.cols = (uint32_t)qx + 1;
  g.rows = (uint32_t)qy + 1;
  return g;
}

// A call's block of device scratch, as a rule carved by a ScratchLayout: allocated on the stream, released in stream order by the destructor
struct Scratch {
  pstk::DevBuf buf;
  Scratch() = default;
  Scratch(const ScratchLayout& layout, hipStream_t s, const char* who) { alloc(layout.total(), s, who); }
  template <class T = void> T* alloc(size_t bytes, hipStream_t s, const char* who) {  // (a block that is one region)
    if (buf.alloc(bytes, s) != hipSuccess) throw hip_failure(std::string(who) + ": scratch allocation failed: ");
    return (T*)buf.p;
  }
  template <class T> T* at(size_t offset) { return (T*)((uint8_t*)buf.p + offset); }
};

// Plan execution: `entries` hold per-mapping descriptors with src_col/dst_col already resolved; the function splits them
// into launches of <= PST_PLAN_MAX_ENTRIES, picks the LDS tile and the kernel body, and enqueues on `stream`.
// If an entry has .bounds set, its AABB record {min xyz, max xyz} is written to bounds_out6 (device-accessible); `folded` = where the
// target's Vec3f64 positions of those n points are (the sign of a zero bound, pstk::ZeroScan).
void execute_entries(bool src_aos, uint64_t src_base, uint32_t src_stride, bool dst_aos, uint64_t dst_base, uint32_t dst_stride,
                     uint64_t n, const std::vector<PlanEntry>& entries, bool allow_lds, hipStream_t stream, double* bounds_out6 = nullptr,
                     bool whole_records_in_place = false, const pstk::ZeroScan& folded = pstk::ZeroScan{0, 0, 0});
bool specialised_kernel_ready(bool src_aos, uint64_t src_base, uint32_t src_stride, bool dst_aos, uint64_t dst_base, uint32_t dst_stride, uint64_t n,
                              const std::vector<PlanEntry>& entries, bool with_bounds);

// identity (same datatype, no transformation) entry between two members
PlanEntry identity_entry(const Member& src, const Member& dst);

void stream_sync(hipStream_t s);
// every byte of a caller's result array, in device (stream-ordered) or in host memory
inline void fill_result(void* p, int byte, size_t bytes, bool on_device, hipStream_t s) {
  if (on_device) PST_HIP_CHECK(hipMemsetAsync(p, byte, bytes, s));
  else std::memset(p, byte, bytes);
}
// OwningBuffer::resize; zero_fill = false leaves new points uninitialised (callers that overwrite every byte)
void resize_buffer(pst_buffer& b, size_t count, bool zero_fill);

// {min xyz, max xyz} of POSITION_3D over points [first, first+count) written to out6 (device-accessible); seeds
// +/-f64::MAX (bounds.rs:31-32).  The buffer must have a Position3D attribute.
size_t bounds_partials_scratch_bytes(size_t count);
void bounds_of_range(const pst_buffer& b, size_t first, size_t count, double* out6, hipStream_t stream, void* partials = nullptr);
// AABB::from_min_max (math/bounds.rs:21-26): throws PST_ERR_BOUNDS_INVALID if min > max on any axis
void check_bounds_record(const double r[6], double out_min[3], double out_max[3]);

}  // namespace pst
