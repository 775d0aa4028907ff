// pst_polygon_set_* / pst_points_in_polygons_device / pst_polygon_mask_device / pst_buffer_set_u8_from_ids_device / pst_crop_kernel_shape:
// argument checks, the polygon set's device memory and the one launch of a query (crop.hip, where the definition and the argument for the box
// tests are; the index is polygon_index.hpp's, built on the host).
#include <cstring>

#include "polygon_index.hpp"
#include "runtime.hpp"

using namespace pst;

// The set owns ONE block of device memory from the driver (not the stream-ordered pool: pst_release_scratch cannot reach it), holding what
// the kernel it takes reads -- flat: the entries' records | their polygon indices; banded: the band lists' records | their polygon indices |
// the band offsets.  The caller's arrays are not kept.
struct pst_polygon_set {
  uint32_t n_polygons = 0, kernel = 0;  // kernel: 1 flat, 2 banded
  uint64_t n_entries = 0, directory_entries = 0;
  pstk::CropSet set{};
  void* block = nullptr;
  ~pst_polygon_set() {
    if (block) (void)hipFree(block);
  }
};

namespace {

// one query: the launch, and the read-back of the count when the caller wants it
void run_query(const pst_polygon_set& ps, const pst_buffer& b, const Member& pm, uint32_t* d_ids, uint8_t* d_mask, int outside, uint64_t* count, const char* who) {
  hipStream_t s = current_stream();
  Scratch block;
  unsigned long long* d_count = nullptr;
  if (count) {
    d_count = block.alloc<unsigned long long>(256, s, who);
    PST_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(*d_count), s));
  }
  if (!pstk::crop_query(positions_of(b, pm), ps.set, ps.kernel == 1, d_ids, d_mask, outside, d_count, s)) throw hip_failure(std::string(who) + ": launch failed: ");
  if (count) {
    unsigned long long selected = 0;
    PST_HIP_CHECK(hipMemcpyAsync(&selected, d_count, sizeof(selected), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    *count = selected;
  }
}

}  // namespace

extern "C" {

int pst_crop_kernel_shape(uint32_t* flat_points_per_block, uint32_t* banded_points_per_block, uint32_t* flat_max_edges) {
  if (flat_points_per_block) *flat_points_per_block = pstk::kCropFlatPointsPerBlock;
  if (banded_points_per_block) *banded_points_per_block = pstk::kCropBandedPointsPerBlock;
  if (flat_max_edges) *flat_max_edges = pstk::kCropFlatMaxEdges;
  return PST_OK;
}

int pst_polygon_set_create(const double* xy, const uint64_t* ring_offsets, size_t n_rings, const uint32_t* polygon_of_ring, uint32_t bands, uint32_t kernel,
                           pst_polygon_set** out) {
  PST_API_BEGIN
  const std::string who = "pst_polygon_set_create";
  not_null(out, "out");
  *out = nullptr;
  not_null(xy, "xy");
  not_null(ring_offsets, "ring_offsets");
  if (kernel > 2) throw Error(PST_ERR_INVALID_ARGUMENT, who + ": kernel must be 0 (automatic), 1 (flat) or 2 (banded)");
  const polygon::Index ix = polygon::build(xy, ring_offsets, n_rings, polygon_of_ring, bands);  // (a refusal: PST_ERR_INVALID_ARGUMENT with its message)
  const size_t n_entries = ix.entries.size();
  if (kernel == 1 && n_entries > pstk::kCropFlatMaxEdges)
    throw Error(PST_ERR_INVALID_ARGUMENT, who + ": the flat kernel takes at most " + std::to_string(pstk::kCropFlatMaxEdges) + " entries, the set has " + std::to_string(n_entries));
  ensure_device();

  std::unique_ptr<pst_polygon_set> ps(new pst_polygon_set);
  ps->n_polygons = ix.n_polygons;
  ps->n_entries = n_entries;
  ps->directory_entries = ix.band_entries.size();
  ps->kernel = kernel ? kernel : (n_entries <= pstk::kCropFlatMaxEdges ? 1u : 2u);
  const bool flat = ps->kernel == 1;
  const size_t n_records = flat ? n_entries : ix.band_entries.size(), n_offsets = flat ? 0 : ix.band_offsets.size();
  const size_t off_polygon = up256(n_records * sizeof(polygon::Entry)), off_offsets = off_polygon + up256(n_records * 4), bytes = off_offsets + up256(n_offsets * 4) + 256;
  std::vector<uint8_t> host(bytes, 0);
  polygon::Entry* records = (polygon::Entry*)host.data();
  uint32_t* pol = (uint32_t*)(host.data() + off_polygon);
  for (size_t k = 0; k < n_records; ++k) {
    const size_t e = flat ? k : ix.band_entries[k];
    records[k] = ix.entries[e];
    pol[k] = ix.polygon[e];
  }
  if (n_offsets) std::memcpy(host.data() + off_offsets, ix.band_offsets.data(), n_offsets * 4);
  PST_HIP_CHECK(dev_malloc_retry(&ps->block, bytes));
  PST_HIP_CHECK(hipMemcpy(ps->block, host.data(), bytes, hipMemcpyHostToDevice));  // synchronous: the set is complete when this returns
  uint8_t* base = (uint8_t*)ps->block;
  ps->set.records = (const double*)base;
  ps->set.polygon = (const uint32_t*)(base + off_polygon);
  ps->set.offsets = flat ? nullptr : (const uint32_t*)(base + off_offsets);
  ps->set.n_records = (uint32_t)n_records;  // (at most 2^27)
  ps->set.bands = ix.bands.count;
  ps->set.xmin = ix.box[0];
  ps->set.ymin = ix.box[1];
  ps->set.xmax = ix.box[2];
  ps->set.ymax = ix.box[3];
  ps->set.scale = ix.bands.scale;
  *out = ps.release();
  PST_API_END
}

int pst_polygon_set_destroy(pst_polygon_set* set) {
  PST_API_BEGIN
  delete set;
  PST_API_END
}

int pst_polygon_set_info(const pst_polygon_set* set, uint64_t counts[4], double box[4], uint32_t* kernel) {
  PST_API_BEGIN
  not_null(set, "set");
  if (counts) {
    counts[0] = set->n_polygons;
    counts[1] = set->n_entries;
    counts[2] = set->set.bands;
    counts[3] = set->directory_entries;
  }
  if (box) {
    box[0] = set->set.xmin;
    box[1] = set->set.ymin;
    box[2] = set->set.xmax;
    box[3] = set->set.ymax;
  }
  if (kernel) *kernel = set->kernel;
  PST_API_END
}

int pst_points_in_polygons_device(const pst_polygon_set* set, const pst_buffer* b, uint32_t* d_ids) {
  PST_API_BEGIN
  const char* who = "pst_points_in_polygons_device";
  not_null(set, "set");
  not_null(b, "buffer");
  const Member& pm = position_member(*b);
  if (b->len == 0) return PST_OK;
  not_null(d_ids, "d_ids");
  ensure_device();
  check_point_count(b->len, who);
  run_query(*set, *b, pm, d_ids, nullptr, 0, nullptr, who);
  PST_API_END
}

int pst_polygon_mask_device(const pst_polygon_set* set, const pst_buffer* b, int outside, uint8_t* d_mask, uint64_t* count) {
  PST_API_BEGIN
  const char* who = "pst_polygon_mask_device";
  not_null(set, "set");
  not_null(b, "buffer");
  const Member& pm = position_member(*b);
  if (count) *count = 0;
  if (b->len == 0) return PST_OK;
  not_null(d_mask, "d_mask");
  ensure_device();
  check_point_count(b->len, who);
  run_query(*set, *b, pm, nullptr, d_mask, outside, count, who);
  PST_API_END
}

int pst_buffer_set_u8_from_ids_device(pst_buffer* b, const char* attribute_name, const uint32_t* d_ids, const uint8_t* d_values, uint32_t n_values, uint64_t* written) {
  PST_API_BEGIN
  const char* who = "pst_buffer_set_u8_from_ids_device";
  not_null(b, "buffer");
  not_null(attribute_name, "attribute_name");
  const Member& m = required(b->layout.find(AttributeDef{attribute_name, DataType{}}));  // (a default datatype is U8)
  if (written) *written = 0;
  if (b->len == 0 || n_values == 0) return PST_OK;  // no point, or no id that names a value: nothing is written
  not_null(d_ids, "d_ids");
  not_null(d_values, "d_values");
  ensure_device();
  hipStream_t s = current_stream();
  Scratch block;
  unsigned long long* d_written = nullptr;
  if (written) {
    d_written = block.alloc<unsigned long long>(256, s, who);
    PST_HIP_CHECK(hipMemsetAsync(d_written, 0, sizeof(*d_written), s));
  }
  const AttrView v = attr_view(*b, &m);
  if (!pstk::set_u8_from_ids(v.addr, v.stride, b->len, d_ids, d_values, n_values, d_written, s)) throw hip_failure(std::string(who) + ": launch failed: ");
  if (written) {
    unsigned long long hits = 0;
    PST_HIP_CHECK(hipMemcpyAsync(&hits, d_written, sizeof(hits), hipMemcpyDeviceToHost, s));
    stream_sync(s);
    *written = hits;
  }
  PST_API_END
}

}  // extern "C"
