// Stand-alone driver of pasture_amd/csrc/polygon_index.hpp (host only, no HIP) for tests/test_polygon_index.py, which builds it under the
// address and undefined-behaviour sanitizers.
//   test_polygon_index <set file> <bands>   builds the index of the set in the file and prints it: the entries and every band's list
//   test_polygon_index refusals             checks that every invalid set is refused with a message, and the limits by their names
// The set file: "<n_rings> <with polygon_of_ring: 0 | 1>", then per ring "<polygon> <m>" and m lines "<x> <y>" (hexadecimal floats).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "polygon_index.hpp"

using namespace pst::polygon;

static int failures = 0;

static void refused(const char* what, const char* needle, const double* xy, const uint64_t* offsets, size_t n_rings, const uint32_t* polygon_of_ring, uint32_t bands) {
  try {
    (void)build(xy, offsets, n_rings, polygon_of_ring, bands);
    std::printf("FAIL: %s was accepted\n", what);
    ++failures;
  } catch (const Refused& e) {
    if (!std::strstr(e.what(), needle)) {
      std::printf("FAIL: %s was refused with '%s', which does not say '%s'\n", what, e.what(), needle);
      ++failures;
    }
  }
}

static int check_refusals() {
  const double square[8] = {0, 0, 1, 0, 1, 1, 0, 1};
  const uint64_t one[2] = {0, 4};
  refused("NULL xy", "NULL", nullptr, one, 1, nullptr, 0);
  refused("NULL ring_offsets", "NULL", square, nullptr, 1, nullptr, 0);
  refused("no ring", "at least one ring", square, one, 0, nullptr, 0);
  const uint64_t from_one[2] = {1, 4}, two_vertices[2] = {0, 2}, decreasing[3] = {0, 4, 3};
  refused("offsets from 1", "start at 0", square, from_one, 1, nullptr, 0);
  refused("a ring of 2 vertices", "at least 3 vertices", square, two_vertices, 1, nullptr, 0);
  refused("decreasing offsets", "at least 3 vertices", square, decreasing, 2, nullptr, 0);
  double bad[8];
  for (const double v : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()})
    for (int at = 0; at < 8; at += 3) {
      std::memcpy(bad, square, sizeof(bad));
      bad[at] = v;
      refused("a vertex that is not finite", "finite", bad, one, 1, nullptr, 0);
    }
  const double two_squares[16] = {0, 0, 1, 0, 1, 1, 0, 1, 2, 0, 3, 0, 3, 1, 2, 1};
  const uint64_t two[3] = {0, 4, 8};
  const uint32_t from_1[2] = {1, 1}, gap[2] = {0, 2}, down[2] = {0, 0};
  refused("polygon_of_ring from 1", "polygon_of_ring", two_squares, two, 2, from_1, 0);
  refused("polygon_of_ring with a gap", "polygon_of_ring", two_squares, two, 2, gap, 0);
  // the limits, by name.  The vertex limit is checked on the OFFSETS: xy is not read (it holds one square)
  const uint64_t too_many[2] = {0, (1ull << 24) + 1};
  refused("2^24 + 1 vertices", "2^24 vertices", square, too_many, 1, nullptr, 0);
  refused("2^24 + 1 bands", "2^24 bands", square, one, 1, nullptr, (1u << 24) + 1);
  // 4098 edges from y = 0 to y = 1, each listed in every band: 4098 * 32768 > 2^27 directory entries -- counted, never allocated
  std::vector<double> zigzag;
  for (int i = 0; i < 4098; ++i) {
    zigzag.push_back((double)i);
    zigzag.push_back((double)(i % 2));
  }
  const uint64_t zz[2] = {0, 4098};
  refused("more than 2^27 directory entries", "2^27 directory entries", zigzag.data(), zz, 1, nullptr, 32768);
  try {  // ... which the automatic choice never runs into, and a caller's B just below the limit is taken
    const Index a = build(zigzag.data(), zz, 1, nullptr, 0);
    if (a.entries.size() != 4098 || a.band_entries.size() != (size_t)4098 * a.bands.count) {
      std::printf("FAIL: the zigzag under automatic bands: %zu entries, %zu directory entries, %u bands\n", a.entries.size(), a.band_entries.size(), a.bands.count);
      ++failures;
    }
    const Index b = build(two_squares, two, 2, down, 1u << 24);
    if (b.bands.count != (1u << 24) || b.n_polygons != 1 || b.entries.size() != 4) {
      std::printf("FAIL: 2^24 bands\n");
      ++failures;
    }
  } catch (const Refused& e) {
    std::printf("FAIL: a valid set was refused: %s\n", e.what());
    ++failures;
  }
  if (!failures) std::printf("refusals honoured\n");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "refusals")) return check_refusals();
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <set file> <bands> | refusals\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  size_t n_rings = 0;
  int with_polygons = 0;
  if (std::fscanf(f, "%zu %d", &n_rings, &with_polygons) != 2) return 2;
  std::vector<double> xy;
  std::vector<uint64_t> offsets{0};
  std::vector<uint32_t> polygon_of_ring;
  for (size_t r = 0; r < n_rings; ++r) {
    uint32_t p = 0;
    size_t m = 0;
    if (std::fscanf(f, "%" SCNu32 " %zu", &p, &m) != 2) return 2;
    polygon_of_ring.push_back(p);
    for (size_t i = 0; i < 2 * m; ++i) {
      char word[64];
      if (std::fscanf(f, "%63s", word) != 1) return 2;
      xy.push_back(std::strtod(word, nullptr));
    }
    offsets.push_back(offsets.back() + m);
  }
  std::fclose(f);
  try {
    const Index ix = build(xy.data(), offsets.data(), n_rings, with_polygons ? polygon_of_ring.data() : nullptr, (uint32_t)std::strtoul(argv[2], nullptr, 10));
    std::printf("polygons %u entries %zu bands %u directory %zu ymin %a scale %a box %a %a %a %a\n", ix.n_polygons, ix.entries.size(), ix.bands.count, ix.band_entries.size(),
                ix.bands.ymin, ix.bands.scale, ix.box[0], ix.box[1], ix.box[2], ix.box[3]);
    for (size_t e = 0; e < ix.entries.size(); ++e)
      std::printf("entry %zu %u %a %a %a %a\n", e, ix.polygon[e], ix.entries[e].lox, ix.entries[e].loy, ix.entries[e].hix, ix.entries[e].hiy);
    if (ix.band_offsets.size() != (size_t)ix.bands.count + 1 || ix.band_offsets[0] != 0 || ix.band_offsets.back() != ix.band_entries.size()) {
      std::printf("FAIL: the offsets do not frame the lists\n");
      return 1;
    }
    for (uint32_t b = 0; b < ix.bands.count; ++b) {
      if (ix.band_offsets[b + 1] < ix.band_offsets[b]) {
        std::printf("FAIL: the offsets decrease at band %u\n", b);
        return 1;
      }
      if (ix.band_offsets[b + 1] == ix.band_offsets[b]) continue;  // (an empty band is not printed)
      std::printf("band %u", b);
      for (uint32_t k = ix.band_offsets[b]; k < ix.band_offsets[b + 1]; ++k) std::printf(" %u", ix.band_entries[k]);
      std::printf("\n");
    }
  } catch (const Refused& e) {
    std::printf("refused: %s\n", e.what());
    return 3;
  }
  std::printf("done\n");
  return 0;
}
