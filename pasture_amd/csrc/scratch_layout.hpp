// Carving a call's one block of device scratch into regions.  No HIP here: the owner of the block is pst::Scratch (runtime.hpp), and
// tests/cpp/test_scratch_layout.cpp includes this header alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pst {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ScratchLayout {
  size_t end = 0;
  // the offset of a new region of `bytes`: every region starts on a 256-byte boundary, and one of 0 bytes takes no room
  size_t add(size_t bytes) {
    const size_t off = end;
    end += up256(bytes);
    return off;
  }
  size_t total() const { return end; }
};

}  // namespace pst
