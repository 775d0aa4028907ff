// The index of a polygon set for the point-in-polygon kernels (crop.hip; include/pasture_amd.h, "Polygon crop and overlay"): plain C++, host
// only, no HIP -- tests/cpp/test_polygon_index.cpp builds it alone under the sanitizers.  Four steps:
//   1. validate the rings and their offsets (every limit is checked on the OFFSETS, before a vertex is read)
//   2. the canonical edge entries: an edge a -> b with a.y == b.y is dropped; every other one is stored as {lo.x, lo.y, hi.x, hi.y}, lo the
//      endpoint with the smaller y, plus the index of its polygon.  Entries keep the input order, so they are sorted by polygon.
//   3. the bounding box of ALL vertices (those of dropped edges included: a larger box is still a box)
//   4. the y-band directory in CSR form: B equal bands over [ymin, ymax], band_entries[band_offsets[b] .. band_offsets[b + 1]) = the entries
//      listed in band b, in input order -- that is, sorted by polygon index, then by input order.
//
// The band of a y is ONE expression, band_of below: t = (y - ymin) * scale, scale = B / (ymax - ymin) rounded once on the host; then floor and
// clamp to [0, B - 1] (t below 1, a NaN t included, is band 0).  The band kernel applies the same function to p.y, and an edge is listed in the
// bands band_of(lo.y) .. band_of(hi.y) by that very function.  Why this is conservative WITHOUT an epsilon: a rounded subtraction of a
// constant, a rounded multiplication by a constant that is not negative, the floor and the clamp are each monotone (not decreasing) in y, so
// band_of is.  A point that can cross an edge has lo.y <= p.y < hi.y, hence band_of(lo.y) <= band_of(p.y) <= band_of(hi.y): the edge is in the
// list of the point's band, whatever the roundings were.  (The one value where t is a NaN is y == ymin with an infinite scale -- a box without
// height: it maps to band 0, below every other y's band, and such a set has no entry at all.)
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define PST_POLYGON_HD __host__ __device__
#else
#define PST_POLYGON_HD
#endif

namespace pst {
namespace polygon {

constexpr uint64_t kMaxVertices = 1ull << 24;          // 2^24 vertices in a set
constexpr uint64_t kMaxDirectoryEntries = 1ull << 27;  // 2^27 entries in all band lists together
constexpr uint32_t kMaxBands = 1u << 24;               // bands a caller may ask for
constexpr uint32_t kMaxAutoBands = 1u << 16;           // bands the automatic choice takes at the most
constexpr uint32_t kAutoEntriesPerBand = 8;            // automatic: one band per this many entries

struct Entry { double lox, loy, hix, hiy; };  // 32 bytes: what the kernels read as one aligned record

struct Bands { double ymin, scale; uint32_t count; };

PST_POLYGON_HD inline uint32_t band_of(const Bands& b, double y) {
  const double t = (y - b.ymin) * b.scale;
  return t >= 1.0 ? (t >= (double)b.count ? b.count - 1 : (uint32_t)t) : 0u;
}

struct Index {
  uint32_t n_polygons = 0;
  std::vector<Entry> entries;
  std::vector<uint32_t> polygon;  // per entry
  double box[4] = {0.0, 0.0, 0.0, 0.0};  // xmin, ymin, xmax, ymax
  Bands bands{0.0, 0.0, 1};
  std::vector<uint32_t> band_offsets;  // bands.count + 1
  std::vector<uint32_t> band_entries;  // indices into `entries`
};

// every refusal: the C ABI answers PST_ERR_INVALID_ARGUMENT with this message
struct Refused : std::invalid_argument {
  using std::invalid_argument::invalid_argument;
};

inline uint64_t directory_entries(const std::vector<Entry>& entries, const Bands& b) {
  uint64_t total = 0;
  for (const Entry& e : entries) total += (uint64_t)(band_of(b, e.hiy) - band_of(b, e.loy)) + 1;
  return total;
}

// xy: the vertices, x and y interleaved, ring after ring; ring r = vertices ring_offsets[r] .. ring_offsets[r + 1] (ring_offsets: n_rings + 1
// values from 0); polygon_of_ring: NULL = one polygon of all rings, else not decreasing from 0 without gaps; bands: 0 = automatic
inline Index build(const double* xy, const uint64_t* ring_offsets, size_t n_rings, const uint32_t* polygon_of_ring, uint32_t bands) {
  const std::string who = "polygon set: ";
  if (!xy || !ring_offsets) throw Refused(who + "xy and ring_offsets must not be NULL");
  if (n_rings == 0) throw Refused(who + "a set has at least one ring");
  if (bands > kMaxBands) throw Refused(who + "more than 2^24 bands");
  if (ring_offsets[0] != 0) throw Refused(who + "ring_offsets must start at 0");
  for (size_t r = 0; r < n_rings; ++r) {
    if (ring_offsets[r + 1] < ring_offsets[r] || ring_offsets[r + 1] - ring_offsets[r] < 3) throw Refused(who + "a ring has at least 3 vertices and ring_offsets do not decrease");
    if (ring_offsets[r + 1] > kMaxVertices) throw Refused(who + "more than 2^24 vertices");
    if (polygon_of_ring) {
      const uint32_t before = r ? polygon_of_ring[r - 1] : 0;
      if (r == 0 ? polygon_of_ring[0] != 0 : (polygon_of_ring[r] != before && polygon_of_ring[r] != before + 1))
        throw Refused(who + "polygon_of_ring must start at 0 and go up in steps of 0 or 1");
    }
  }
  const uint64_t n_vertices = ring_offsets[n_rings];
  Index ix;
  ix.n_polygons = polygon_of_ring ? polygon_of_ring[n_rings - 1] + 1 : 1;
  double xmin = xy[0], ymin = xy[1], xmax = xy[0], ymax = xy[1];
  for (uint64_t v = 0; v < n_vertices; ++v) {
    const double x = xy[2 * v], y = xy[2 * v + 1];
    if (!std::isfinite(x) || !std::isfinite(y)) throw Refused(who + "every vertex must be finite");
    xmin = x < xmin ? x : xmin;
    xmax = x > xmax ? x : xmax;
    ymin = y < ymin ? y : ymin;
    ymax = y > ymax ? y : ymax;
  }
  ix.box[0] = xmin;
  ix.box[1] = ymin;
  ix.box[2] = xmax;
  ix.box[3] = ymax;
  for (size_t r = 0; r < n_rings; ++r) {
    const uint64_t first = ring_offsets[r], m = ring_offsets[r + 1] - first;
    for (uint64_t i = 0; i < m; ++i) {
      const double* a = xy + 2 * (first + i);
      const double* b = xy + 2 * (first + (i + 1 == m ? 0 : i + 1));  // closed implicitly, last vertex to first
      if (a[1] == b[1]) continue;
      const bool a_is_lo = a[1] < b[1];
      ix.entries.push_back(a_is_lo ? Entry{a[0], a[1], b[0], b[1]} : Entry{b[0], b[1], a[0], a[1]});
      ix.polygon.push_back(polygon_of_ring ? polygon_of_ring[r] : 0u);
    }
  }
  const uint64_t n_entries = ix.entries.size();
  ix.bands.ymin = ymin;
  const auto with_count = [&](uint32_t count) {
    ix.bands.count = count;
    ix.bands.scale = (double)count / (ymax - ymin);  // (a box without height: +inf, and no entry; an extent that overflows: 0, one band in effect)
    return directory_entries(ix.entries, ix.bands);
  };
  uint64_t total = 0;
  if (bands) {
    total = with_count(bands);
    if (total > kMaxDirectoryEntries) throw Refused(who + "more than 2^27 directory entries: ask for fewer bands");
  } else {  // one band per kAutoEntriesPerBand entries, halved while the lists together would be too long (one band lists every entry once: that fits)
    uint64_t count = (n_entries + kAutoEntriesPerBand - 1) / kAutoEntriesPerBand;
    count = count < 1 ? 1 : (count > kMaxAutoBands ? kMaxAutoBands : count);
    while ((total = with_count((uint32_t)count)) > kMaxDirectoryEntries) count /= 2;
  }
  // CSR by counting: the entries are walked in input order both times, so every band's list keeps that order
  ix.band_offsets.assign((size_t)ix.bands.count + 1, 0u);
  for (const Entry& e : ix.entries)
    for (uint32_t b = band_of(ix.bands, e.loy), last = band_of(ix.bands, e.hiy); b <= last; ++b) ++ix.band_offsets[b + 1];
  for (uint32_t b = 0; b < ix.bands.count; ++b) ix.band_offsets[b + 1] += ix.band_offsets[b];
  ix.band_entries.resize(total);
  std::vector<uint32_t> at(ix.band_offsets.begin(), ix.band_offsets.end() - 1);
  for (uint64_t e = 0; e < n_entries; ++e)
    for (uint32_t b = band_of(ix.bands, ix.entries[e].loy), last = band_of(ix.bands, ix.entries[e].hiy); b <= last; ++b) ix.band_entries[at[b]++] = (uint32_t)e;
  return ix;
}

}  // namespace polygon
}  // namespace pst
