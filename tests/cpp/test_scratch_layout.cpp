// The scratch carver of the RANSAC, outlier and cluster entry points (pasture_amd/csrc/scratch_layout.hpp), on the host alone:
// tests/test_scratch_layout.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <vector>

#include "scratch_layout.hpp"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }  // the expression the entry points used to spell out

int main() {
  using pst::ScratchLayout;

  {  // an empty layout
    ScratchLayout l;
    CHECK(l.total() == 0);
    CHECK(l.add(0) == 0);
    CHECK(l.total() == 0);
  }

  {  // sizes around the boundary: the offsets are the cumulative rounding, in every order of the four sizes
    const size_t sizes[4] = {1, 255, 256, 257};
    for (int rot = 0; rot < 4; ++rot) {
      ScratchLayout l;
      size_t expected = 0;
      for (int i = 0; i < 4; ++i) {
        const size_t v = sizes[(i + rot) % 4];
        CHECK(l.add(v) == expected);
        expected += round256(v);
        CHECK(l.total() == expected);
      }
    }
    ScratchLayout l;
    CHECK(l.add(1) == 0);
    CHECK(l.add(255) == 256);
    CHECK(l.add(256) == 512);
    CHECK(l.add(257) == 768);
    CHECK(l.total() == 1280);
  }

  {  // a mixed sequence with empty regions in it: aligned, in order, no overlap, total = rounded end of the last region
    const std::vector<size_t> sizes = {24, 0, 4096, 1, 0, 0, 64, 257, 1000003, 0, 255, 8};
    ScratchLayout l;
    size_t last_end = 0;  // the end (not rounded) of the last region that has bytes
    for (size_t bytes : sizes) {
      const size_t before = l.total();
      const size_t off = l.add(bytes);
      CHECK(off % 256 == 0);
      CHECK(off >= last_end);  // regions in order never overlap
      CHECK(off == before);    // a new region starts at the running end ...
      if (bytes == 0) {
        CHECK(l.total() == before);  // ... and an empty one adds nothing
      } else {
        last_end = off + bytes;
        CHECK(l.total() >= last_end);
        CHECK(l.total() == round256(last_end));
      }
      CHECK(l.total() % 256 == 0);
    }
    CHECK(l.total() == round256(last_end));
    const size_t end = l.total();
    CHECK(l.add(0) == end && l.add(0) == end && l.total() == end);
  }

  {  // the "only when the caller does not supply it" regions: leaving one out moves what follows down by its rounded size, nothing else
    for (size_t n : {size_t(1), size_t(255), size_t(256), size_t(257), size_t(100000)}) {
      ScratchLayout with, without;
      const size_t a0 = with.add(n * 12), a1 = with.add(n * 8), a2 = with.add(64), a3 = with.add(n);
      const size_t b0 = without.add(n * 12), b1 = without.add(0), b2 = without.add(64), b3 = without.add(0);
      CHECK(a0 == b0 && a1 == b1);
      CHECK(a2 == b2 + round256(n * 8));
      CHECK(b3 == without.total());
      CHECK(with.total() == a3 + round256(n));
      CHECK(without.total() == b2 + 256);
    }
  }

  {  // what the halves of the cluster call rely on: in the 4-byte unit b4 = up256((n + 1) * 4), an 8-byte array of n + 1 elements fits 2 * b4
    for (size_t n : {size_t(1), size_t(63), size_t(64), size_t(255), size_t(256), size_t(257), size_t(0xFFFFFFEF)}) {
      const size_t b4 = pst::up256((n + 1) * 4), room8 = pst::up256((n + 1) * 8);
      CHECK(b4 == round256((n + 1) * 4));
      CHECK(room8 <= 2 * b4);
      CHECK((n + 1) * 4 <= b4);  // the second half, b4 bytes in, starts behind the first half's elements
      ScratchLayout l;  // and carved as the call carves them, two 8-byte arrays then a 4-byte one
      CHECK(l.add(2 * b4) == 0);
      CHECK(l.add(2 * b4) == 2 * b4);
      CHECK(l.add(b4) == 4 * b4);
      CHECK(l.total() == 5 * b4);
    }
  }

  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
