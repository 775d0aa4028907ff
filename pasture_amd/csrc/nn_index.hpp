// The persistent nearest-neighbour index behind the C ABI's pst_nn_index: built and searched by nn_api.cpp, read by m3c2_api.cpp.
#pragma once
#include "runtime.hpp"

// The index owns ONE block of device memory from the driver (not the stream-ordered pool, not a call's scratch: pst_release_scratch cannot
// reach it): sorted keys | xs | ys | zs | buffer index of every sorted position, for the nf finite targets.  Nothing of the target buffer is
// kept: the index is valid after the buffer has changed or gone.
// Target normals (pst_nn_index_set_normals*) live in a SECOND block from the driver, nx | ny | nz in the same sorted order, 24 bytes per
// finite target; an index over a target without a finite point accepts normals and holds none.  An all-zero pst_nn_index is an index over
// an empty target without normals (the host-side tests stand one up that way).
struct pst_nn_index {
  pstk::NnGrid grid{};
  uint32_t nf = 0;
  uint64_t occupied = 0;
  void* block = nullptr;
  uint64_t* keys = nullptr;
  double *xs = nullptr, *ys = nullptr, *zs = nullptr;
  uint32_t* order = nullptr;
  uint64_t n_target = 0;  // the target's length at creation: what a set of normals must have
  bool has_normals = false;
  void* normals_block = nullptr;
  double *nx = nullptr, *ny = nullptr, *nz = nullptr;
  void drop_normals() {
    if (normals_block) (void)hipFree(normals_block);
    normals_block = nullptr;
    nx = ny = nz = nullptr;
    has_normals = false;
  }
  ~pst_nn_index() {
    if (block) (void)hipFree(block);
    if (normals_block) (void)hipFree(normals_block);
  }
};
