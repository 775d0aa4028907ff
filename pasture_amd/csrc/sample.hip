// Minimum-distance (Poisson-disk) subsampling: the mask of the sequential greedy pass "in ascending priority key, keep a finite point iff no
// kept point conflicts with it", conflict = (dx*dx + dy*dy) + dz*dz <= r2 (include/pasture_amd.h, "Minimum-distance subsampling"; every
// operation a separately rounded f64 operation, no sqrt -- the adjacency of clusters.hip).
//
// Pipeline (sample_api.cpp drives it; the host reads one small record, then one count per round):
//   bounds    AABB over the FINITE points and their number: block partials, then one folding workgroup -- no atomics
//   keys      cluster_keys of clusters.hip on the same grid (cell edge STRICTLY above the radius by the relative margin 2^-20: the argument at
//             the head of clusters.hip carries over word for word, conflicting points are at most one cell apart on every axis), the 64-bit
//             radix sort, then the positions gathered into sorted order.  From here on a point's id is its SORTED position s < nf.
//   decide    the hot kernel, one lane per ACTIVE (still undecided) point: all nine (y, z) rows of the 3 x 3 x 3 stencil, each one contiguous
//             key range [x - 1, x + 1] found by two binary searches of the sorted keys (the cell of a key, the rows, the search and the
//             predicate are grid_index_device.hpp's; DBSCAN's count and border kernels walk the same way).  Among the conflicting candidates
//             of SMALLER priority key: a kept one makes the point rejected (stop at the first); otherwise, if none is undecided, the point is kept; otherwise it
//             stays undecided.  A lane sweeps its point kSampleSweepsPerLaunch times at the most.
//   compact   flags (1 = still undecided, written by the decision kernel) -> exclusive scan -> the next active list; the host reads its length
//   mask      mask[order[s]] = state[s] == kept for s < nf, 0 for the non-finite points behind them; the kept count
//
// Memory ordering.  One state byte per sorted point: undecided (0), kept (1), rejected (2).  States are read with agent-scope relaxed atomic
// loads and written with agent-scope relaxed atomic stores; no fences, no ordering between different bytes is needed.  A lane may see decisions
// made in the same launch.  That is safe: a state only ever LEAVES "undecided" (one store per point, by the one lane that owns it), and a lane
// decides only from FINAL states -- it rejects on a candidate read as kept, it keeps when every conflicting candidate of smaller key was read as
// rejected.  By induction on the priority key every state that is ever stored is the greedy pass's: the smallest key has no smaller conflict
// and is kept; a point whose smaller conflicts all carry greedy states is rejected iff one of them is kept, which is the greedy rule.  A read
// that is stale (the XCDs' L2s are not coherent) returns an earlier value of the byte, and the only earlier value is "undecided": the lane
// stays undecided where it could have decided, which costs a round, never correctness.  Every launch decides at least the undecided point of
// smallest key (all its smaller conflicts were final before the launch began, and a launch sees what the launches before it wrote), so the
// loop of rounds ends; the result depends on nothing but the predicate and the keys -- not on the grid, the schedule or the number of rounds.
//
// Traffic per candidate: the state byte first (a rejected candidate costs nothing more -- from the second round on most are), then the three
// coordinates (24 bytes), then, only where it conflicts, its buffer index (4 bytes) from which the priority key is recomputed (ten integer
// operations); storing the keys next to the positions would read 8 bytes there instead and write 8 bytes per point in the gather.
#include "grid_index_device.hpp"

using namespace pstd;

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kP = pstk::kSamplePointsPerBlock;
constexpr uint32_t kSweeps = pstk::kSampleSweepsPerLaunch;
constexpr uint32_t kBP = pstk::kSampleBoundsPointsPerBlock;
static_assert(kP == kBlock, "one lane per point");

enum : uint8_t { kUndecided = 0, kKept = 1, kRejected = 2 };

using Bounds = pstk::SampleBounds;
using Grid = pstk::ClusterGrid;

// ---- bounds -----------------------------------------------------------------------------------------------------------------------------------
// thread 0 leaves with the block's fold
__device__ __forceinline__ void block_fold(double (&mn)[3], double (&mx)[3], unsigned long long& c, double* sv, unsigned long long* sc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += shfl_xor_any(c, off);
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
  block_reduce_minmax<double, 3>(mn, mx, sv);  // (its barrier publishes sc as well)
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t w = 1; w < kBlock / 64; ++w) c += sc[w];
  }
}

__global__ __launch_bounds__(kBlock) void sample_bounds_partial_kernel(Pos pos, uint64_t n, Bounds* __restrict__ partials) {
  __shared__ double sv[4 * 2 * 3];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kBP;
  double mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
  unsigned long long c = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < kBP / kBlock; ++j) {
    const uint64_t i = first + j * kBlock + threadIdx.x;
    if (i >= n) continue;
    double x, y, z;
    load_point(pos, i, x, y, z);
    if (!(finite(x) && finite(y) && finite(z))) continue;
    mn[0] = fold_min(mn[0], x); mn[1] = fold_min(mn[1], y); mn[2] = fold_min(mn[2], z);
    mx[0] = fold_max(mx[0], x); mx[1] = fold_max(mx[1], y); mx[2] = fold_max(mx[2], z);
    c += 1;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) partials[blockIdx.x] = Bounds{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}, c};
}

// ONE workgroup: thread t folds the contiguous run [t * per, (t + 1) * per) of the block partials, then the same tree
__global__ __launch_bounds__(kBlock) void sample_bounds_final_kernel(const Bounds* __restrict__ partials, uint64_t blocks, Bounds* __restrict__ rec) {
  __shared__ double sv[4 * 2 * 3];
  __shared__ unsigned long long sc[kBlock / 64];
  const uint64_t per = (blocks + kBlock - 1) / kBlock, b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  double mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
  unsigned long long c = 0;
  for (uint64_t b = b0; b < b1; ++b) {
    const Bounds p = partials[b];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fold_min(mn[a], p.min[a]);
      mx[a] = fold_max(mx[a], p.max[a]);
    }
    c += p.count;
  }
  block_fold(mn, mx, c, sv, sc);
  if (threadIdx.x == 0) *rec = Bounds{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}, c};
}

// ---- the decision -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// the priority key of buffer index i (include/pasture_amd.h): shuffled = splitmix64(seed ^ i), index order = i
__device__ __forceinline__ unsigned long long priority_of(uint32_t shuffled, unsigned long long seed, uint32_t i) {
  return shuffled ? splitmix64(seed ^ (unsigned long long)i) : (unsigned long long)i;
}

__device__ __forceinline__ uint8_t state_of(const uint8_t* state, uint32_t s) { return __hip_atomic_load(state + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// active == nullptr: the first round, every sorted point is active (m == nf).  flags: m + 1 entries, flags[t] = 1 iff active point t leaves
// the launch undecided, flags[m] = 0 (the scan's last offset is their number).
__global__ __launch_bounds__(kBlock) void sample_decide_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ xs, const double* __restrict__ ys,
                                                               const double* __restrict__ zs, const uint32_t* __restrict__ order, uint32_t nf, Grid g, double r2,
                                                               uint32_t shuffled, unsigned long long seed, const uint32_t* __restrict__ active, uint32_t m,
                                                               uint8_t* state, uint32_t* __restrict__ flags) {
  const uint32_t t = blockIdx.x * kP + threadIdx.x;
  if (t >= m) return;
  if (t == m - 1) flags[m] = 0;
  const uint32_t s = active ? active[t] : t;
  const Cell cell = cell_of_key(keys[s], g);
  const double px = xs[s], py = ys[s], pz = zs[s];
  const unsigned long long mine = priority_of(shuffled, seed, order[s]);
  uint8_t st = kUndecided;
#pragma unroll 1
  for (uint32_t sweep = 0; sweep < kSweeps && st == kUndecided; ++sweep) {
    bool kept_seen = false, undecided_seen = false;
#pragma unroll 1
    for (int r = 0; r < 9 && !kept_seen; ++r) {
      unsigned long long row;
      if (!stencil_row(cell, g, r / 3 - 1, r % 3 - 1, row)) continue;
      const uint32_t first = lower_bound(keys, nf, row | cell.x0);
      const uint32_t last = lower_bound(keys, nf, (row | cell.x1) + 1);
      for (uint32_t c = first; c < last; ++c) {
        if (c == s) continue;
        const uint8_t sc = state_of(state, c);
        if (sc == kRejected) continue;  // a rejected point decides nothing
        if (!(squared_distance(xs[c], ys[c], zs[c], px, py, pz) <= r2)) continue;
        if (priority_of(shuffled, seed, order[c]) > mine) continue;  // (keys never tie: both orders are injective in the buffer index)
        if (sc == kKept) { kept_seen = true; break; }
        undecided_seen = true;
      }
    }
    if (kept_seen) st = kRejected;
    else if (!undecided_seen) st = kKept;
    // stored here, inside the loop: the lanes of this wave that sweep once more are to see it
    if (st != kUndecided) __hip_atomic_store(state + s, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  flags[t] = st == kUndecided ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void sample_compact_kernel(const uint32_t* __restrict__ active, const uint32_t* __restrict__ flags,
                                                                const unsigned long long* __restrict__ offsets, uint32_t m, uint32_t* __restrict__ next) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= m || !flags[t]) return;
  next[offsets[t]] = active ? active[t] : t;  // offsets[t] < the number of flagged entries <= m
}

// ---- the mask ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sample_mask_kernel(const uint32_t* __restrict__ order, const uint8_t* __restrict__ state, uint64_t n, uint32_t nf,
                                                             uint8_t* __restrict__ mask, unsigned long long* __restrict__ kept) {
  __shared__ uint32_t sc[kBlock / 64];
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool k = s < nf && state[s] == kKept;
  if (s < n) mask[order[s]] = k ? 1 : 0;  // (the non-finite points sorted behind the finite ones)
  const uint32_t in_wave = (uint32_t)__builtin_popcountll(__ballot(k));
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = in_wave;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) c += sc[w];
    if (c) atomicAdd(kept, (unsigned long long)c);
  }
}

}  // namespace

namespace pstk {

static unsigned bounds_blocks(uint64_t n) { return blocks_of(n, kBP); }
size_t sample_bounds_partials_bytes(uint64_t n) { return (size_t)(bounds_blocks(n) ? bounds_blocks(n) : 1u) * sizeof(SampleBounds); }

bool sample_bounds(const Positions& pos, void* partials, SampleBounds* rec, hipStream_t stream) {
  const unsigned blocks = bounds_blocks(pos.n);
  if (blocks) hipLaunchKernelGGL(sample_bounds_partial_kernel, dim3(blocks), dim3(kBlock), 0, stream, pos_of(pos), pos.n, (SampleBounds*)partials);
  hipLaunchKernelGGL(sample_bounds_final_kernel, dim3(1), dim3(kBlock), 0, stream, (const SampleBounds*)partials, (uint64_t)blocks, rec);
  return launched();
}

bool sample_decide(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint32_t* order, uint32_t nf, const ClusterGrid& g,
                   double r2, uint32_t shuffled, uint64_t seed, const uint32_t* active, uint32_t m, uint8_t* state, uint32_t* flags, hipStream_t stream) {
  if (m == 0) return true;
  hipLaunchKernelGGL(sample_decide_kernel, dim3(blocks_of(m, kP)), dim3(kBlock), 0, stream, sorted_keys, xs, ys, zs, order, nf, g, r2, shuffled, (unsigned long long)seed,
                     active, m, state, flags);
  return launched();
}

bool sample_compact(const uint32_t* active, const uint32_t* flags, const unsigned long long* offsets, uint32_t m, uint32_t* next, hipStream_t stream) {
  if (m == 0) return true;
  hipLaunchKernelGGL(sample_compact_kernel, dim3(blocks_of(m, kBlock)), dim3(kBlock), 0, stream, active, flags, offsets, m, next);
  return launched();
}

bool sample_mask(const uint32_t* order, const uint8_t* state, uint64_t n, uint32_t nf, uint8_t* mask, unsigned long long* kept, hipStream_t stream) {
  if (n == 0) return true;
  hipLaunchKernelGGL(sample_mask_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, stream, order, state, n, nf, mask, kept);
  return launched();
}

}  // namespace pstk
