// Individual trees: tree tops by a local-maximum filter and crowns after Silva et al. 2016 (include/pasture_amd.h, "Individual trees").
//
// Definitions.  Height h_i = z of point i, or heights[i] when a column is given (z is then not read).  A point is VALID when x, y and h are
// finite and its mask byte is not zero.  Candidates C = the valid points with h >= min_height.  r_i = min(max(a + b*h_i, r_min), r_max);
// j is in i's window iff dx*dx + dy*dy <= r_i*r_i, dx = x_j - x_i, dy = y_j - y_i; j DOMINATES i iff h_j > h_i, or h_j == h_i and j < i in
// buffer order.  Candidate i is a top iff no other candidate in ITS window dominates it.  Every operation a separately rounded f64 operation.
//
// The index is dense_grid_device.hpp's over the members a byte selects, with a third column: x, y, h as three f64 arrays next to the buffer
// index of every sorted position, and the dense directory.  The sort, the directory heads and the suffix minimum are the library's launches
// (dense_directory.hpp); the member pass, the keys and the gather are here because the height may come from a column and z must then not be
// looked at (hag.hip's test all three components).
//
// The filter, exactness.  A dominator of i is a candidate in i's window.  trees_window.hpp argues from the roundings of the predicate that
// every point the ROUNDED predicate accepts lies in a cell of the box trees_window_cells returns, whatever the edge (its steps 1 - 5).  The
// near pass tests the intersection of that box with the 3 x 3 cells around i: a dominator found there is a dominator (it is tested with the
// predicate itself), and when the box lies inside the 3 x 3 cells the pass has seen every cell a dominator could be in.  Every other
// candidate goes to the far pass, which tests every cell of the box.  Both test `dominates` first and the distance second: two compares
// decide most candidates.  Neither the order of the tests nor the cells visited enter the result: a candidate is a top iff NO member of a
// set that contains every dominator is one.
// Why two passes: in a canopy most candidates lose to a neighbour of their own cell, one lane each is the right shape for them, and a
// wave's lanes -- neighbours in cell order -- leave early together.  A top must see its whole window: hundreds of candidates, which one lane
// would walk with 63 idle beside it; the far pass gives it a wave, the lanes across a row's candidates.
//
// The crown search, exactness.  It is the ring walk of dense_grid_device.hpp with k = 1 over an index of the tops, the bound B the best d2
// so far, which starts at m2 = rc_max * rc_max: the argument there covers it.  What is new is the bound: rc_t = half_factor * H_t and
// rc_max = half_factor * max |H|.  Multiplication by a fixed non-negative factor and squaring of |.| are monotone under rounding, so
// rc_t*rc_t <= rc_max*rc_max = m2 for every top: a top beyond m2 fails its own test d2 <= rc_t*rc_t, and when the nearest top of all lies
// beyond m2 the point is unlabelled either way.  (max |H|, not max H: a top of negative height has a positive rc*rc too.)
#include "dense_grid_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kTreesPointsPerBlock;
constexpr uint32_t kS = pstk::kTreesSurvivorsPerBlock;
constexpr uint32_t kQ = pstk::kTreesQueriesPerBlock;
constexpr uint32_t kBP = pstk::kTreesBoundsPointsPerBlock;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kP == kBlock, "one lane per candidate");
static_assert(kS * 64 == kBlock, "one wave per survivor");
static_assert(kQ == 64, "the crown search is written for one wave per workgroup");
static_assert(kBP % kBlock == 0, "a thread of the member pass takes kBP / kBlock points");

using Grid = pstk::HagGrid;
using Bounds = pstk::TreesBounds;
using Window = pstk::TreeWindow;

// pstk::TreesInput as the kernels take it
struct In { Pos pos; const double* heights; const uint8_t* mask; };
inline In in_of(const pstk::TreesInput& in) { return In{pos_of(in.pos), in.heights, in.mask}; }

__device__ __forceinline__ void load_xyh(const In& in, uint64_t i, double& x, double& y, double& h) {
  cgptr_t q = in.pos.base + i * in.pos.stride;
  x = load_un<double>(q);
  y = load_un<double>(q + 8);
  h = in.heights ? in.heights[i] : load_un<double>(q + 16);
}
__device__ __forceinline__ bool valid(const In& in, uint64_t i, double x, double y, double h) {
  return finite(x) && finite(y) && finite(h) && (!in.mask || in.mask[i]);
}
__device__ __forceinline__ bool dominates(double hj, uint32_t j, double hi, uint32_t i) { return hj > hi || (hj == hi && j < i); }

// ---- members: the byte, and the block partials of their bounds ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void trees_members_kernel(In in, uint64_t n, const uint8_t* __restrict__ also, double floor, uint8_t* __restrict__ member,
                                                               Bounds* __restrict__ partials) {
  __shared__ double sv[4 * 2 * 3];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kBP;
  // slot 2: unused by the minima, max |h| by the maxima
  double mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
  unsigned long long c = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < kBP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    double x, y, h;
    load_xyh(in, i, x, y, h);
    const bool m = valid(in, i, x, y, h) && (!also || also[i]) && h >= floor;
    member[i] = m ? 1 : 0;
    if (!m) continue;
    mn[0] = fold_min(mn[0], x); mn[1] = fold_min(mn[1], y);
    mx[0] = fold_max(mx[0], x); mx[1] = fold_max(mx[1], y); mx[2] = fold_max(mx[2], __builtin_fabs(h));
    c += 1;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) partials[blockIdx.x] = Bounds{mn[0], mn[1], mx[0], mx[1], mx[2], c};
}

// ONE workgroup: thread t folds the contiguous run [t * per, (t + 1) * per) of the block partials, then the same tree
__global__ __launch_bounds__(kBlock) void trees_members_final_kernel(const Bounds* __restrict__ partials, uint64_t blocks, Bounds* __restrict__ rec) {
  __shared__ double sv[4 * 2 * 3];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t per = (blocks + kBlock - 1) / kBlock, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
  unsigned long long c = 0;
  for (uint64_t b = b0; b < b1; ++b) {
    const Bounds p = partials[b];
    mn[0] = fold_min(mn[0], p.min_x); mn[1] = fold_min(mn[1], p.min_y);
    mx[0] = fold_max(mx[0], p.max_x); mx[1] = fold_max(mx[1], p.max_y); mx[2] = fold_max(mx[2], p.max_abs_h);
    c = c + p.count;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) *rec = Bounds{mn[0], mn[1], mx[0], mx[1], mx[2], c};
}

// ---- keys and gather --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void trees_key_kernel(Pos pos, const uint32_t* __restrict__ subset, const uint8_t* __restrict__ member, uint64_t count, Grid g,
                                                           uint32_t* __restrict__ keys) {
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= count) return;
  const uint64_t i = subset ? subset[e] : e;
  uint32_t key = no_member_key(g);
  if (!member || member[i]) {
    cgptr_t q = pos.base + i * pos.stride;
    key = member_key(load_un<double>(q), load_un<double>(q + 8), g);
  }
  keys[e] = key;
}

__global__ __launch_bounds__(kBlock) void trees_gather_kernel(In in, const uint32_t* __restrict__ subset, const uint32_t* __restrict__ order, uint32_t m,
                                                              double* __restrict__ xs, double* __restrict__ ys, double* __restrict__ hs, uint32_t* __restrict__ index) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t i = subset ? subset[order[s]] : order[s];
  double x, y, h;
  load_xyh(in, i, x, y, h);
  xs[s] = x; ys[s] = y; hs[s] = h;
  if (index) index[s] = i;
}

// ---- the local-maximum filter -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void trees_near_kernel(Window w, Grid g, const uint32_t* __restrict__ dir, const double* __restrict__ xs, const double* __restrict__ ys,
                                                            const double* __restrict__ hs, const uint32_t* __restrict__ index, uint32_t nc, uint8_t* __restrict__ top_mask,
                                                            uint32_t* __restrict__ flags) {
  const uint32_t s = blockIdx.x * kP + threadIdx.x;
  if (s >= nc) return;
  if (s == nc - 1) flags[nc] = 0;
  const double x = xs[s], y = ys[s], h = hs[s];
  const uint32_t i = index[s];
  const double r = pstk::trees_window_radius(w, h);
  const double r2 = r * r;
  const pstk::TreeCellBox box = pstk::trees_window_cells(x, y, r, g);
  const uint32_t cx = cell_of(x, g.min[0], g.edge, g.dim[0]), cy = cell_of(y, g.min[1], g.edge, g.dim[1]);
  // the 3 x 3 cells, clipped to the box (which holds the own cell: the cell expression is monotone and reach >= 0)
  const uint32_t xa = cx > box.x0 ? cx - 1 : box.x0, xb = cx < box.x1 ? cx + 1 : box.x1;
  const uint32_t ya = cy > box.y0 ? cy - 1 : box.y0, yb = cy < box.y1 ? cy + 1 : box.y1;
  bool dominated = false;
#pragma unroll 1
  for (uint32_t yy = ya; yy <= yb && !dominated; ++yy) {
    const uint32_t row = yy * g.dim[0];  // below 2^26
    const uint32_t first = dir[row + xa], last = dir[row + xb + 1];
    for (uint32_t c = first; c < last; ++c) {
      if (!dominates(hs[c], index[c], h, i)) continue;  // (the candidate itself does not dominate itself)
      const double dx = xs[c] - x, dy = ys[c] - y;
      const double d2 = dx * dx + dy * dy;
      if (d2 <= r2) { dominated = true; break; }
    }
  }
  const bool whole = xa == box.x0 && xb == box.x1 && ya == box.y0 && yb == box.y1;
  if (!dominated && whole) top_mask[i] = 1;
  flags[s] = (!dominated && !whole) ? 1u : 0u;
}

template <bool kWork>
__global__ __launch_bounds__(kBlock) void trees_far_kernel(Window w, Grid g, const uint32_t* __restrict__ dir, const double* __restrict__ xs, const double* __restrict__ ys,
                                                           const double* __restrict__ hs, const uint32_t* __restrict__ index, const uint32_t* __restrict__ survivors,
                                                           uint32_t m, uint8_t* __restrict__ top_mask, unsigned long long* __restrict__ work) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t t = blockIdx.x * kS + (threadIdx.x >> 6);  // wave-uniform
  if (t >= m) return;
  const uint32_t s = survivors[t];
  const double x = xs[s], y = ys[s], h = hs[s];
  const uint32_t i = index[s];
  const double r = pstk::trees_window_radius(w, h);
  const double r2 = r * r;
  const pstk::TreeCellBox box = pstk::trees_window_cells(x, y, r, g);
  bool dominated = false;
  unsigned long long tested = 0;
#pragma unroll 1
  for (uint32_t yy = box.y0; yy <= box.y1 && !dominated; ++yy) {
    const uint32_t row = yy * g.dim[0];
    const uint32_t first = dir[row + box.x0], last = dir[row + box.x1 + 1];  // the same two words in every lane
#pragma unroll 1
    for (uint32_t base = first; base < last; base += 64) {
      const uint32_t c = base + lane;
      bool hit = false;
      if (c < last && dominates(hs[c], index[c], h, i)) {
        const double dx = xs[c] - x, dy = ys[c] - y;
        const double d2 = dx * dx + dy * dy;
        hit = d2 <= r2;
      }
      if (kWork) tested += last - base < 64 ? last - base : 64;
      if (__ballot(hit)) { dominated = true; break; }  // (wave-uniform)
    }
  }
  if (lane == 0) {
    if (!dominated) top_mask[i] = 1;
    if (kWork && tested) atomicAdd(work, tested);
  }
}

// ---- the numbering ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void trees_flags_kernel(const uint8_t* __restrict__ bytes, uint64_t n, uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n) return;
  flags[i] = (i < n && bytes[i]) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void trees_list_kernel(In in, const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ offsets, uint64_t n,
                                                            unsigned long long* __restrict__ keys, uint32_t* __restrict__ list) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || !flags[i]) return;
  double x, y, h;
  load_xyh(in, i, x, y, h);
  const unsigned long long at = offsets[i];
  keys[at] = ~ordered(h + 0.0);  // taller first; -0.0 + 0.0 is +0.0: the two zeros tie, and the stable sort keeps the lower index in front
  list[at] = (uint32_t)i;
}

// ---- the crown search -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void trees_query_key_kernel(In in, uint64_t n, double floor, Grid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x, y, h;
  load_xyh(in, i, x, y, h);
  keys[i] = valid(in, i, x, y, h) && h >= floor ? query_key(x, y, g) : no_member_key(g);  // (no query: behind every query)
  vals[i] = (uint32_t)i;
}

// the best (d2, buffer index of the top, sorted position) so far: hag.hip's list with k = 1, all of it in registers
struct Best { double d2; uint32_t idx, at; };

__device__ __forceinline__ void scan(const double* __restrict__ xs, const double* __restrict__ ys, const uint32_t* __restrict__ index, uint32_t first, uint32_t last, double qx,
                                     double qy, Best& b) {
  for (uint32_t c = first; c < last; ++c) {
    const double dx = xs[c] - qx, dy = ys[c] - qy;
    const double d2 = dx * dx + dy * dy;
    if (d2 <= b.d2) {
      const uint32_t j = index[c];
      if (d2 < b.d2 || j < b.idx) { b.d2 = d2; b.idx = j; b.at = c; }
    }
  }
}

// counts[t] += 1 for the lane's tree t (kNone: nothing).  EVERY lane of the wave gets here.  The lanes of a wave are neighbours and mostly
// share a tree: those that share the first pending lane's fold their count in the wave and send one atomic (grid_index_device.hpp's tally,
// counts only); after four distinct trees the lanes still pending send their own.  Integer sums: the grouping cannot matter.
__device__ __forceinline__ void tally_tree(uint32_t t, uint32_t* counts) {
  bool pending = t != kNone;
#pragma unroll 1
  for (uint32_t round = 0; round < 4; ++round) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;  // (wave-uniform)
    const int leader = __builtin_ctzll(todo);
    const uint32_t t0 = (uint32_t)__shfl((int)t, leader, 64);
    const bool same = pending && t == t0;
    const uint32_t members = (uint32_t)__builtin_popcountll(__ballot(same));
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(counts + t0, members);
    pending = pending && !same;
  }
  if (pending) atomicAdd(counts + t, 1u);
}

__global__ __launch_bounds__(kQ) void trees_crown_kernel(In in, uint32_t nq, Grid g, double m2, double half_factor, double exclusion, const uint32_t* __restrict__ qkeys,
                                                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ dir, const double* __restrict__ xs,
                                                         const double* __restrict__ ys, const double* __restrict__ hs, const uint32_t* __restrict__ index,
                                                         const uint32_t* __restrict__ number, uint32_t* __restrict__ ids, uint32_t* __restrict__ counts,
                                                         unsigned long long* __restrict__ labelled) {
  const uint32_t lane = threadIdx.x;
  const uint32_t s = blockIdx.x * kQ + lane;
  uint32_t id = kNone;
  if (s < nq) {
    const uint32_t i = order[s];
    const uint32_t key = qkeys[s];
    if (is_member_key(key, g)) {  // a query
      double qx, qy, qh;
      load_xyh(in, i, qx, qy, qh);
      Best b{m2, kNone, kNone};
      uint32_t cx, cy;
      cell_of_key(key, g, cx, cy);
      walk_rings(g, dir, cx, cy, [&](uint32_t first, uint32_t last) { scan(xs, ys, index, first, last, qx, qy, b); }, [&] { return b.d2; });
      if (b.at != kNone) {  // the nearest top first, then its two tests
        const double H = hs[b.at];
        const double rc = half_factor * H;
        const double floor_h = exclusion * H;
        if (b.d2 <= rc * rc && qh >= floor_h) id = number[b.at];
      }
    }
    ids[i] = id;
  }
  tally_tree(id, counts);
  const unsigned long long c = (unsigned long long)__popcll(__ballot(id != kNone));
  if (lane == 0 && c) atomicAdd(labelled, c);
}

}  // namespace

namespace pstk {

size_t trees_bounds_partials_bytes(uint64_t n) { return (size_t)(blocks_of(n, kBP) ? blocks_of(n, kBP) : 1u) * sizeof(TreesBounds); }

bool trees_members(const TreesInput& in, const uint8_t* also, double floor, uint8_t* member, void* partials, TreesBounds* rec, hipStream_t stream) {
  const unsigned blocks = blocks_of(in.pos.n, kBP);
  if (blocks) hipLaunchKernelGGL(trees_members_kernel, dim3(blocks), dim3(kBlock), 0, stream, in_of(in), in.pos.n, also, floor, member, (TreesBounds*)partials);
  hipLaunchKernelGGL(trees_members_final_kernel, dim3(1), dim3(kBlock), 0, stream, (const TreesBounds*)partials, (uint64_t)blocks, rec);
  return launched();
}

bool trees_keys(const Positions& pos, const uint32_t* subset, const uint8_t* member, uint64_t count, const HagGrid& g, uint32_t* keys, hipStream_t stream) {
  if (count == 0) return true;
  hipLaunchKernelGGL(trees_key_kernel, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, stream, pos_of(pos), subset, member, count, g, keys);
  return launched();
}

bool trees_gather(const TreesInput& in, const uint32_t* subset, const uint32_t* order, uint32_t m, double* xs, double* ys, double* hs, uint32_t* index, hipStream_t stream) {
  if (m == 0) return true;
  hipLaunchKernelGGL(trees_gather_kernel, dim3(blocks_of(m, kBlock)), dim3(kBlock), 0, stream, in_of(in), subset, order, m, xs, ys, hs, index);
  return launched();
}

bool trees_filter_near(const TreeWindow& w, const HagGrid& g, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index, uint32_t nc,
                       uint8_t* top_mask, uint32_t* flags, hipStream_t stream) {
  if (nc == 0) return true;
  hipLaunchKernelGGL(trees_near_kernel, dim3(blocks_of(nc, kP)), dim3(kBlock), 0, stream, w, g, dir, xs, ys, hs, index, nc, top_mask, flags);
  return launched();
}

bool trees_filter_far(const TreeWindow& w, const HagGrid& g, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index,
                      const uint32_t* survivors, uint32_t m, uint8_t* top_mask, unsigned long long* work, hipStream_t stream) {
  if (m == 0) return true;
  if (work) hipLaunchKernelGGL(trees_far_kernel<true>, dim3(blocks_of(m, kS)), dim3(kBlock), 0, stream, w, g, dir, xs, ys, hs, index, survivors, m, top_mask, work);
  else hipLaunchKernelGGL(trees_far_kernel<false>, dim3(blocks_of(m, kS)), dim3(kBlock), 0, stream, w, g, dir, xs, ys, hs, index, survivors, m, top_mask, work);
  return launched();
}

bool trees_flags(const uint8_t* bytes, uint64_t n, uint32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(trees_flags_kernel, dim3(blocks_of(n + 1, kBlock)), dim3(kBlock), 0, stream, bytes, n, flags);
  return launched();
}

bool trees_list(const TreesInput& in, const uint32_t* flags, const unsigned long long* offsets, uint64_t n, unsigned long long* keys, uint32_t* list, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(trees_list_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, in_of(in), flags, offsets, n, keys, list);
  return launched();
}

bool trees_query_keys(const TreesInput& in, double floor, const HagGrid& g, uint32_t* keys, uint32_t* vals, hipStream_t stream) {
  if (in.pos.n == 0) return true;
  hipLaunchKernelGGL(trees_query_key_kernel, dim3(blocks_of(in.pos.n, kBlock)), dim3(kBlock), 0, stream, in_of(in), in.pos.n, floor, g, keys, vals);
  return launched();
}

bool trees_crown_search(const TreesInput& in, uint32_t n, const HagGrid& g, double m2, double half_factor, double exclusion, const uint32_t* query_keys,
                        const uint32_t* query_order, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index,
                        const uint32_t* number, uint32_t* ids, uint32_t* counts, unsigned long long* labelled, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(trees_crown_kernel, dim3(blocks_of(n, kQ)), dim3(kQ), 0, stream, in_of(in), n, g, m2, half_factor, exclusion, query_keys, query_order, dir, xs, ys, hs,
                     index, number, ids, counts, labelled);
  return launched();
}

}  // namespace pstk
