// Host-callable launchers of the gfx950 kernels (implemented in *.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pasture_amd.h"
#include "cluster_grid.hpp"
#include "hag_grid.hpp"
#include "trees_window.hpp"
#include "plan.h"

namespace pstk {

// K2/K3/K3' generic conversion.  src_aos / dst_aos select the interleaved arms of buffer_conversion.rs:418-662.
// use_lds: stage interleaved records through LDS tiles (plan.tile must be set); otherwise direct strided access.
// Returns false when the launch (or the plan upload) failed; inspect hipGetLastError().
// n_records: number of per-block AABB records written behind plan.h.bounds_partials (plans with fused bounds).
bool launch_convert(const ConvertPlan& plan, bool src_aos, bool dst_aos, bool use_lds, hipStream_t stream, unsigned* n_records = nullptr);
// upper bound of those records: a plan with fused bounds needs room for convert_max_records() records of 6 doubles (+ finalize room)
unsigned convert_max_records(const ConvertPlan& plan, bool src_aos, bool dst_aos, bool use_lds);
// which kernel families (PST_PLAN_* bits) the calling thread's last conversion call launched
void reset_plan_kinds();
void note_plan_kind(uint32_t kind);
uint32_t plan_kinds();
// One note on stderr per process and `what` when a call of 2^20 points or more ends on a fall-back kernel family (the interpreter, the gather
// kernels): those run at 0.26-0.70 of peak where the plan-specialised families reach 0.75-0.84, and a caller who never asks
// pst_last_plan_kinds would not know.  PST_QUIET=1 silences it.
void note_slow_family(const char* what, uint64_t n_points, const char* why);
// compile (or fetch) the plan-specialised kernel this plan would take (jit.cpp); false + message when it cannot have one
bool prepare_convert(const ConvertPlan& plan, bool src_aos, bool dst_aos, std::string* error, bool* in_tree = nullptr);
bool launch_convert_fused_expressions(const ConvertPlan& plan, bool src_aos, bool dst_aos, hipStream_t stream, uint64_t* done, std::string* error);
bool convert_specialised_ready(const ConvertPlan& plan, bool src_aos, bool dst_aos);
size_t bounds_partials_bytes(unsigned n_records);
// The elements a fold ran over, for the sign of a bound that comes out as +-0 (zero_sign.hpp): element e's components at base + e * stride.
// n = 0: none (the bound keeps whichever zero the fold returned).
struct ZeroScan { uint64_t base, stride, n; };
// fold n_records per-block {min xyz, max xyz} records into out6; `folded` = the Vec3f64 values those records were folded from
void launch_finalize_bounds(double* partials, unsigned n_records, double* out6, hipStream_t stream, const ZeroScan& folded);
// pst_bounds_record_set_form: records at these addresses leave the last fold kernel as {min, -max}
void set_bounds_record_form(const void* device_rec6, int form);
bool bounds_record_negates_max(const void* device_rec6);
int device_cus();
// Dynamic LDS bytes of a launch that needs `lds_bytes` and wants at most `resident` workgroups per CU (0 = whatever fits): the memory side of
// MI355X saturates with FEW bytes in flight per CU and loses throughput beyond that (profiles/r05_stream_sweeps.txt), so the streaming kernels
// cap their residency by asking for more LDS than they use.  PST_RESIDENT=<n> overrides every family's cap (same-box A/Bs; 0 = no cap).
// Never more than 64 KiB (no per-kernel attribute needed): caps below 2 are not expressible this way.
uint32_t lds_with_resident_cap(size_t lds_bytes, int resident);
constexpr int kResidentQuad = 0;          // plan-specialised conversion kernels (one-wave workgroups, 256-point tiles)
constexpr int kResidentFilterStream = 0;  // plan-specialised streaming compaction
constexpr int kResidentColumn = 4;        // columnar -> columnar conversion of one attribute (columns.hip) when the loads are the 16-byte side:
                                          // f64 -> f32 narrowing at 10^8 points 0.776 -> 0.801 of peak, 8 of 8 ABAB pairs (profiles/r05_abab.txt)

// K1/K2 fast path: columnar Vec3f64 stream. mode bits: 1 = affine, 2 = write dst, 4 = bounds.
// partials must hold stream_partials_bytes(); out6 receives {min xyz, max xyz} when bounds are requested.
// Modes 2 (plain copy) and 5 (bounds of the transformed values, nothing written) have no caller in the library; tests/test_stream_seams.py runs
// them.  Mode 5 looks up the sign of a +-0 bound (zero_sign.hpp) in the UNTRANSFORMED source, the only values in memory: such a bound is zero by
// value, its sign is not the index-order sign of the transformed values.
int stream_grid();
size_t stream_partials_bytes(uint64_t n_points, unsigned mode);  // bytes `partials` must hold for this launch
void launch_vec3f64_stream(const double* src, double* dst, uint64_t n_points, const double scale[3], const double offset[3],
                           unsigned mode, double* partials, double* out6, hipStream_t stream);

// generic strided min/max over elements of `ncomp` components of component type `ct`.
// acc_f64: accumulate in f64 after a Rust `as` cast (calculate_bounds_from_custom_positions) with +/-f64::MAX seeds;
// otherwise accumulate in the component type with identity seeds.  out holds 2*ncomp accumulators {min.., max..}.
int reduce_grid();
size_t minmax_partials_bytes();
void launch_minmax(const uint8_t* base, uint64_t stride, uint64_t n, uint32_t ct, uint32_t ncomp, bool acc_f64, void* partials,
                   void* out, hipStream_t stream);

// Where a call's positions are: Vec3f64 at base + i * stride, for n points (pst::positions_of makes it; kernels read it through positions_device.hpp)
struct Positions { const uint8_t* base; uint64_t stride; uint64_t n; };

// compute_centroid (normal_estimation.rs:198-237): per-block records {sum xyz over all points, sum xyz over the finite points, finite count,
// NaN seen} of Vec3f64 values at base + e * stride; returns the number of records written to `partials` (centroid_partials_bytes())
size_t centroid_partials_bytes();
unsigned launch_centroid(const uint8_t* base, uint64_t stride, uint64_t n, double* partials, hipStream_t stream);

// deterministic synthetic fill of one attribute (see synth.hip)
struct SynthAttr {
  uint64_t base;    // address of the attribute of point 0
  uint64_t stride;  // bytes between points
  uint32_t size;    // attribute bytes
  uint32_t slot;    // index of the attribute in the layout
  uint32_t kind;    // PST_* datatype kind
  uint32_t special; // 0 generic, 1 Position3D, 2 LASLocalPosition, 3 mask 7, 4 mask 1
};
void launch_synth(const SynthAttr& a, uint64_t n, uint64_t seed, uint64_t first_index, hipStream_t stream);

// columnar -> columnar conversion of one attribute (columns.hip): e.src_col / e.dst_col are the range starts.
// With bounds_partials != nullptr (Vec3f64 target) the written values are folded into column_launch_grid() records.
unsigned column_launch_grid(const PlanEntry& e, uint64_t n, bool with_bounds);
bool launch_column(const PlanEntry& e, uint64_t n, double* bounds_partials, hipStream_t stream);

// K4 kNN normal estimation (normals.hip).  Positions: Vec3f64 at pos_base + i*pos_stride.  Outputs (all optional, device
// addresses): normals f64 [n][3], curvature f64 [n], knn int64 [n][k] and / or uint32 [n][k], NORMAL attribute (Vec3f32) and Curvature
// attribute (F64) of a target buffer.  Returns 0, -1 on a HIP failure, -2 beyond 2^32 - 16 points, or the number of neighbourhoods with
// < 3 usable points.
void release_normals_scratch();
struct KnnPlanRecord;  // normals_host.hpp
long long run_normals(const uint8_t* pos_base, uint64_t pos_stride, uint64_t n, uint32_t k, double* out_normals_dev, double* out_curv_dev,
                      long long* out_knn_dev, uint32_t* out_knn_u32_dev, uint64_t normal_attr, uint64_t normal_stride, uint64_t curv_attr,
                      uint64_t curv_stride, hipStream_t stream, KnnPlanRecord* record = nullptr);
// Stream-ordered replay of a recorded call (no host round trip, no allocation: hipGraph-capturable).  KnnPlan owns the scratch of the
// pipeline for its record's capacities; status2 = two device words: [0] = KNN_STATUS_* bits (0: the results are complete and exact),
// [1] = neighbourhoods with fewer than 3 usable points.
struct KnnPlan;
KnnPlan* knn_plan_create(const KnnPlanRecord& rec, bool packed_source, hipStream_t stream);
void knn_plan_free(KnnPlan* p);
const KnnPlanRecord& knn_plan_record(const KnnPlan* p);
// the capacities the plan sized from its record; the counters of its latest replay, copied to the host (synchronises the stream)
struct KnnPlanCaps;
struct KnnReplayCounters;
KnnPlanCaps knn_plan_caps(const KnnPlan* p);
bool knn_plan_read_counters(const KnnPlan* p, KnnReplayCounters& out, hipStream_t stream);
// a plan made on a packed, 8-byte aligned Vec3f64 array searches its source in place and has no staging copy: it replays packed sources only;
// a plan made on any other storage owns a staging copy and replays both
bool knn_plan_accepts(const KnnPlan* p, const uint8_t* pos_base, uint64_t pos_stride);
bool run_normals_replay(KnnPlan* p, const uint8_t* pos_base, uint64_t pos_stride, double* out_normals_dev, double* out_curv_dev, uint32_t* out_knn_u32_dev,
                        uint64_t normal_attr, uint64_t normal_stride, uint64_t curv_attr, uint64_t curv_stride, unsigned long long* status2, hipStream_t stream);

// LAS record encoder (las_encode.hip)
uint32_t las_raw_record_size(int format);
size_t las_encode_workspace_bytes();
bool launch_las_encode(int format, const uint64_t* attr_base, const uint32_t* attr_stride, const uint32_t* attr_size, int n_attrs, bool interleaved,
                       uint64_t dst, uint64_t n,
                       const double scale[3], const double offset[3], const double bounds_in[6], uint32_t max_return, uint8_t* workspace,
                       double* out_bounds, unsigned long long* out_counts, hipStream_t stream);


// LAS record decoder (las_decode.hip)
unsigned las_decode_grid(uint64_t n);
bool launch_las_decode(int format, uint64_t src, uint64_t n, const uint64_t* dst_cols, int n_cols, const double scale[3], const double offset[3],
                       double* partials, hipStream_t stream);
unsigned las_decode_aos_grid(int format, uint64_t n);
bool launch_las_decode_aos(int format, uint64_t src, uint64_t dst, uint64_t n, const double scale[3], const double offset[3], double* partials,
                           hipStream_t stream);

// typed LAS points, columns <-> packed records (las_transpose.hip)
unsigned las_transpose_grid(uint64_t n);
bool launch_las_transpose(int format, bool to_records, uint64_t aos, const uint64_t* cols, int n_cols, uint64_t n, double* partials,
                          hipStream_t stream);

// predicate compaction (filter.hip)
size_t filter_workspace_bytes(uint64_t n);
uint32_t filter_tile(bool dst_aos, uint32_t dst_stride);
bool filter_record_tile_fits(uint32_t tile, uint32_t dst_stride);  // interleaved targets: do 16 records fit the LDS record tile?
void launch_filter_count(const uint8_t* mask_dev, uint64_t n, uint32_t tile, uint8_t* workspace, const unsigned long long** out_total_dev,
                         hipStream_t stream, unsigned long long* total_also = nullptr);
// A predicate fused into the streaming compaction kernel (round 6; expr.cpp writes the text): filter's closure (point_buffer.rs:1064-1136) evaluated by
// the count pass on the columns it names and AGAIN by the scatter pass on the values it holds in registers anyway -- no byte mask in between.
struct FilterPredicate {
  struct Attr { int slot; const char* type_name; uint32_t ncomp; };  // an argument of pst_pred: layout slot, component type (C name), components (1 / 3)
  std::string function_text;  // `PstV3`, and `pst_pred(<the named attributes>, i, p0, p1, p2, p3)`
  std::vector<Attr> attrs;    // in pst_pred's parameter order
  const double* p[4] = {nullptr, nullptr, nullptr, nullptr};
};
// does a compaction of attributes of these sizes take the streaming kernel at all (bytes per point, record size)?  The fused predicate lives there only.
bool filter_predicate_streams(const uint32_t* size, int n_attrs, bool dst_aos, uint32_t dst_stride, bool dst_covered);
std::string filter_stream_source(const uint32_t* size, int n_attrs, bool dst_aos, uint32_t dst_stride, bool dst_covered, const FilterPredicate* pred);  // '' = no streaming kernel
uint32_t* filter_counts(uint8_t* workspace, uint64_t n, uint32_t tile);  // where the scan expects the per-tile counts
void launch_filter_scan(uint64_t n, uint32_t tile, uint8_t* workspace, const unsigned long long** out_total_dev, hipStream_t stream,
                        unsigned long long* total_also = nullptr);
// pred != nullptr: the full tiles through the streaming kernel with the predicate inside (compiled in the calling thread; false + *error when it has
// none), `mask_dev` then covers the ragged last tile only -- rebased so that mask_dev[i] is point i's byte -- and may be null when there is none
bool launch_filter_scatter(const uint8_t* mask_dev, uint64_t n, uint32_t tile, uint8_t* workspace, uint64_t limit, const uint64_t* src_addr,
                           const uint32_t* src_stride, const uint64_t* dst_addr, const uint32_t* dst_off, const uint32_t* size, int n_attrs,
                           bool dst_aos, uint64_t dst_aos_base, uint32_t dst_stride, bool dst_covered, hipStream_t stream,
                           const FilterPredicate* pred = nullptr, std::string* error = nullptr);


// voxel-grid down-sampling (voxel.hip)
enum : uint32_t { VX_AVG_VEC = 1, VX_AVG_NUM = 2, VX_MOST_COMMON = 3, VX_MOST_COMMON_BOOL = 4, VX_MAX_POOL = 5 };
enum : uint32_t { VX_STATUS_BOUNDS_INVALID = 1, VX_STATUS_MARKER_CAPACITY = 2, VX_STATUS_VOXEL_CAPACITY = 4, VX_STATUS_LEAF = 8 };
struct VoxelGridState;
// capacities a stream-ordered plan is built for (voxel_plan_create): points, key bits per axis (>= the bits the marker counts need),
// markers in total, occupied voxels, LDS points per 64-voxel group of the reduction, the leaf sizes
struct VoxelPlanShape { uint64_t n; uint32_t bits[3]; uint32_t cap_markers; uint64_t cap_voxels; uint32_t stage_cap; double leaf[3]; };
VoxelGridState* voxel_plan_create(const VoxelPlanShape& shape, hipStream_t stream);
bool voxel_grid_build_async(VoxelGridState* st, const uint8_t* pos_base, uint64_t pos_stride, const double* bounds6, unsigned long long* count_and_status,
                            hipStream_t stream);
long long voxel_grid_build(VoxelGridState*& st, const uint8_t* pos_base, uint64_t pos_stride, uint64_t n, const double* markers_x, uint32_t nx,
                           const double* markers_y, uint32_t ny, const double* markers_z, uint32_t nz, const double origin[3], const double leaf[3],
                           hipStream_t stream);
bool voxel_grid_reduce(VoxelGridState* st, const uint64_t* src_addr, const uint32_t* src_stride, const uint64_t* dst_addr, const uint32_t* dst_stride,
                       const uint32_t* reduce, const uint32_t* kind, int n_attrs, uint64_t dst_first, hipStream_t stream);
void voxel_grid_free(VoxelGridState* st);


// RANSAC plane / line segmentation (ransac.hip).  The kernels' seams, which the tests place their sizes around (pst_ransac_kernel_shape):
constexpr uint32_t kRansacPointsPerWave = 256;    // one wave scores a tile of this many points, four per lane in registers
constexpr uint32_t kRansacPointsPerBlock = 1024;  // four waves; also the tile of the ordered index compaction
constexpr uint32_t kRansacBlocksPerCu = 8;        // grid = min(blocks needed, CUs x this): one grid pass covers CUs x 8 x 1024 points
constexpr uint32_t kRansacBatch = 1024;           // hypotheses scored per pass over the positions (per-wave LDS counters: 4 KiB)
size_t ransac_record_bytes(bool line);
// table -> scoring (one pass over the positions per kRansacBatch hypotheses) -> arg-max.  recs: iterations records, rank: iterations u64,
// out8: {best iteration, its ranking, model doubles x 6} (64 bytes).  samples_dev: iterations x 3 (plane) / x 2 (line) point indices.
bool ransac_fit(bool line, const Positions& p, double thr, const uint64_t* samples_dev, uint64_t iterations, void* recs, unsigned long long* rank,
                unsigned long long* out8, hipStream_t stream);
// model: plane a b c d / line first xyz, second xyz.  rec_scratch: ransac_record_bytes() of device memory.
bool ransac_model_record(bool line, const double* model, double thr, void* rec_scratch, hipStream_t stream);
bool ransac_mask(bool line, const Positions& p, const double* model, double thr, void* rec_scratch, uint8_t* mask_dev, hipStream_t stream);
// write = false: counts[block] = inliers among the block's kRansacPointsPerBlock points; write = true: the indices, ascending, at offsets[block] ..
bool ransac_index_pass(bool line, const Positions& p, const void* rec, uint32_t* counts, const unsigned long long* offsets, unsigned long long* indices, bool write,
                       hipStream_t stream);

// Neighbour distances and outlier masks over the kNN lists (outliers.hip).  The kernels' seams (pst_outlier_kernel_shape):
constexpr uint32_t kOutlierPointsPerBlock = 64;   // a workgroup of the distance kernels owns the whole lists of this many points, whatever k
constexpr uint32_t kOutlierReduceBlock = 256;     // threads of the one workgroup that adds the block partials, each a contiguous run of them
constexpr uint32_t kOutlierReducePoints = 1024;   // points per block partial of the sums
size_t outlier_record_bytes();                    // the result record: {mean, stddev, threshold, (double)m} as doubles, then the kept count (u64)
size_t outlier_partials_bytes(uint64_t n);
// knn_dev: uint32 [n][k] as run_normals writes them.  dist_dev: f64 [n][k]
bool outlier_distances(const Positions& pos, uint32_t k, const uint32_t* knn_dev, double* dist_dev, hipStream_t stream);
// dbar_dev[q] = (d[q][1] + ... + d[q][mean_k]) / mean_k, mean_k < k
bool outlier_mean_distances(const Positions& pos, uint32_t k, uint32_t mean_k, const uint32_t* knn_dev, double* dbar_dev, hipStream_t stream);
// count and sum -> mean -> squared deviations -> stddev, threshold -> mask and kept count; partials: outlier_partials_bytes(n), record: outlier_record_bytes()
bool outlier_statistics_and_mask(const double* dbar_dev, uint64_t n, double stddev_mult, void* partials, void* record, uint8_t* mask_dev, hipStream_t stream);
// mask[q] = d[q][slot] <= radius; the record's kept count
bool outlier_radius_mask(const Positions& pos, uint32_t k, uint32_t slot, double radius, const uint32_t* knn_dev, void* record, uint8_t* mask_dev,
                         hipStream_t stream);

// Geometric features over the kNN lists (features.hip).  The kernel's seams (pst_features_kernel_shape):
constexpr uint32_t kFeaturesThreads = 256;         // threads of a workgroup
uint32_t features_points_per_block(uint32_t k);    // points whose whole lists one workgroup stages in LDS: 256, 128, 64, 32 for k <= 8, 16, 32, 64
// knn_dev: uint32 [n][k]; out_dev: f64 [planes][n], one plane per bit of `features`; normals_dev, directions_dev: f64 [n][3]; each output nullable
bool geometric_features(const Positions& pos, uint32_t k, const uint32_t* knn_dev, double max_distance, uint32_t features, double* out_dev, double* normals_dev,
                        double* directions_dev, hipStream_t stream);

// Euclidean cluster extraction (clusters.hip; the pipeline and its scratch are laid out in clusters_api.cpp).  The seams (pst_cluster_kernel_shape):
constexpr uint32_t kClusterPointsPerBlock = 256;  // points one workgroup of the traversal kernel owns, one lane each
constexpr uint32_t kClusterTilePoints = 0;        // points of an LDS candidate tile: none, the candidates are read from the sorted arrays
// the device-side record of one call (64 bytes): the AABB of the finite points in the order-preserving integer encoding, their number, the
// points that carry a label (the last two in this order: they are the two counters of the clusters' numbering, cluster_numbering.hpp)
struct ClusterRecord { unsigned long long min_ordered[3], max_ordered[3], finite_count, clustered; };
double cluster_decode_ordered(unsigned long long v);
// (ClusterGrid: cluster_grid.hpp)
bool cluster_bounds(const Positions& pos, ClusterRecord* rec, hipStream_t stream);
// keys[i] = cell key of point i (all ones: not finite), vals[i] = i
bool cluster_keys(const Positions& pos, const ClusterGrid& g, unsigned long long* keys, uint32_t* vals, hipStream_t stream);
// gather (positions of the nf finite points in sorted order, parent[s] = s; `gathered`, optional, is recorded behind it), then traversal + union
// (of `pos` only base and stride are used: the gather reads the nf points `order` names)
bool cluster_components(const Positions& pos, const ClusterGrid& g, double t2, const unsigned long long* sorted_keys, const uint32_t* order, uint32_t nf, double* xs,
                        double* ys, double* zs, uint32_t* parent, hipStream_t stream, hipEvent_t gathered = nullptr);
// root[s], and points and smallest buffer index per root (both set up here; the wave-folded tally of grid_index_device.hpp)
bool cluster_flatten(uint32_t* parent, const uint32_t* order, uint32_t nf, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream);
// The numbering, for the clusters, DBSCAN and the regions alike (cluster_numbering.hpp runs the three in order).  n_ids ids -- sorted positions
// or buffer indices -- carry roots; only a root has root[id] == id; min_index names one of the buffer's n points.
// flags[i] = 1 and root_at[i] = root where i is the smallest member of a component of min_size .. max_size points (flags: n + 1 elements, set up
// here, the last one 0); *n_labelled (zeroed) += the kept sizes
bool cluster_flag_kept(const uint32_t* root, const uint32_t* size, const uint32_t* min_index, uint64_t n, uint32_t n_ids, uint64_t min_size, uint64_t max_size,
                       uint32_t* flags, uint32_t* root_at, unsigned long long* n_labelled, hipStream_t stream);
// offsets = exclusive sum of flags: list_keys[offsets[i]] = 0xFFFFFFFF - size, list_roots[offsets[i]] = root of every flagged i
bool cluster_list_kept(const uint32_t* flags, const unsigned long long* offsets, const uint32_t* root_at, const uint32_t* size, uint64_t n, uint32_t* list_keys,
                       uint32_t* list_roots, hipStream_t stream);
// the list after the stable sort: rank_of_root = 0xFFFFFFFF for all n_ids, then c for root sorted_roots[c]; sizes[c]
bool cluster_ranks(const uint32_t* sorted_keys, const uint32_t* sorted_roots, uint32_t kept, uint32_t n_ids, uint32_t* rank_of_root, unsigned long long* sizes,
                   hipStream_t stream);
// labels[order[s]] = rank of s's root (0xFFFFFFFF: dropped), 0xFFFFFFFF for the non-finite points
bool cluster_labels(const uint32_t* order, const uint32_t* root, const uint32_t* rank_of_root, uint64_t n, uint32_t nf, uint32_t* labels, hipStream_t stream);
bool cluster_mask(const uint32_t* labels, uint64_t n, uint32_t first_cluster, uint32_t cluster_count, uint8_t* mask, hipStream_t stream);

// Ground classification by the progressive morphological filter (pmf.hip; the schedule, the grid and the order of the passes are in pmf_api.cpp).
// The seams (pst_pmf_kernel_shape):
constexpr uint32_t kPmfPointsPerBlock = 1024;  // points per workgroup of the raster, classification and set-where passes, four per lane
constexpr uint32_t kPmfTileCols = 64;          // raster cells one workgroup of a morphology pass writes: one wave per tile row ...
constexpr uint32_t kPmfTileRows = 32;          // ... eight rows per wave
// Largest half-width of ONE morphology pass.  The LDS tile of a pass carries a halo of that many cells on both sides of the axis it works
// along: (kPmfTileRows + 2 H) x kPmfTileCols doubles for the column pass, the larger of the two.  H = 32 makes that 96 x 64 x 8 = 48 KiB:
// static LDS (below 64 KiB), three workgroups per compute unit of its 160 KiB, and every window of the default schedule (up to 16) one pass.
constexpr uint32_t kPmfMaxHalfWidth = 32;
constexpr uint32_t kPmfMaxWindows = 32;
// the raster: cell (row, col) of a point = (trunc((y - y0) / cell), trunc((x - x0) / cell)), rows x cols cells, row-major with col fastest
struct PmfGrid { double x0, y0, cell; uint32_t cols, rows; };
// cells[row * cols + col] = min over the finite points of the cell of the ordered encoding of z; the caller has set every byte of `cells`
bool pmf_raster(const Positions& pos, const PmfGrid& g, unsigned long long* cells, hipStream_t stream);
// One separable pass, out of place: out[r][c] = min (dilate: max over the entries below +inf, +inf without one) of in over |d| <= h along
// the columns (axis 0) or the rows (axis 1), clipped to the raster; h <= kPmfMaxHalfWidth.  in_is_keys: `in` holds pmf_raster's keys (all
// ones = +inf).  fold 1: also L[cell] = out + th; fold 2: L[cell] = min(L[cell], out + th).
bool pmf_morphology_pass(const void* in, bool in_is_keys, double* out, uint32_t cols, uint32_t rows, uint32_t h, bool dilate, int axis, double* L, int fold,
                         double th, hipStream_t stream);
// keys to doubles in place (all ones = +inf)
bool pmf_decode_keys(unsigned long long* cells, uint64_t n_cells, hipStream_t stream);
// mask[i] = 1 iff point i is finite and z <= L[its cell]; *count += the ones (one integer atomic per workgroup)
bool pmf_classify(const Positions& pos, const PmfGrid& g, const double* L, uint8_t* mask, unsigned long long* count, hipStream_t stream);
// mask[i] = 1 iff x, y and z of point i are finite
bool finite_mask(const Positions& pos, uint8_t* mask, hipStream_t stream);
// the byte at addr + i * stride = value wherever mask[i] != 0, i < n
bool set_u8_where(uint64_t addr, uint64_t stride, uint64_t n, const uint8_t* mask, uint8_t value, hipStream_t stream);

// Nearest neighbours between two clouds and the sums of an ICP step (nn.hip; the index and the ICP loop are in nn_api.cpp).  The seams
// (pst_nn_kernel_shape):
constexpr uint32_t kNnQueriesPerBlock = 256;  // queries one workgroup of the search kernel owns, one lane each; candidates are not staged in LDS
constexpr uint32_t kNnReduceBlock = 256;      // threads of the one workgroup that adds the block partials of the ICP sums
constexpr uint32_t kNnReducePoints = 1024;    // source points per block partial
// the cluster grid with the far corner of the AABB (queries are clamped into it) and the edge the ring bound is computed with
struct NnGrid { double min[3], max[3]; double edge, edge_stop; uint32_t dim[3]; uint32_t bits[3]; };
// x' = ((m[0]*x + m[1]*y) + m[2]*z) + m[3], ...; on == 0: the point as it is stored
struct NnTransform { double m[12]; int on; };
// the device-side record of one ICP step
struct NnSums { unsigned long long matched; double cq[3], cp[3], H[9], sum_d2; };
// positions of the nf finite points `order` names, in that order
bool nn_gather(const Positions& pos, const uint32_t* order, uint32_t nf, double* xs, double* ys, double* zs, hipStream_t stream);
// *count = number of different keys among sorted_keys[0, nf)
bool nn_count_cells(const unsigned long long* sorted_keys, uint32_t nf, unsigned long long* count, hipStream_t stream);
// keys[i] = cell key of the transformed query i clamped into the grid's AABB (all ones: not finite), vals[i] = i
bool nn_query_keys(const Positions& pos, const NnTransform& t, const NnGrid& g, unsigned long long* keys, uint32_t* vals, hipStream_t stream);
// query_keys / query_order: the sorted pairs (null, or nf == 0: nothing is searched and every query is unmatched).  Per query, each optional:
// the match's target buffer index, its distance, its position in the index's sorted arrays (0xFFFFFFFF / +inf / 0xFFFFFFFF without a match)
bool nn_search(const Positions& pos, const NnTransform& t, const NnGrid& g, double m2, const unsigned long long* query_keys, const uint32_t* query_order,
               const unsigned long long* keys, const double* xs, const double* ys, const double* zs, const uint32_t* target_index, uint32_t nf, uint32_t* out_idx,
               double* out_dist, uint32_t* out_at, hipStream_t stream);
bool nn_distance_mask(const double* dist, uint64_t n, double threshold, int keep_far, uint8_t* mask, hipStream_t stream);
size_t nn_icp_partials_bytes(uint64_t n);
// at: what nn_search wrote as out_at for these source points and this transform
bool nn_icp_sums(const Positions& pos, const NnTransform& t, const uint32_t* at, const double* xs, const double* ys, const double* zs, const double origin[3],
                 void* partials, NnSums* rec, hipStream_t stream);
// Point-to-plane: the target normals in the index's sorted order, and the sums of a point-to-plane step.
// the device-side record of one point-to-plane step: A the upper triangle of sum j j^T row-major, j = ((q' - cq) x n, n); g = sum j r
struct NnPlaneSums { unsigned long long matched, used; double cq[3], A[21], g[6], sum_r2, sum_w2, sum_d2; };
// nx[s], ny[s], nz[s] = the normal of target order[s], widened to f64: three f64 (is_f32 == false) or three f32 at base + order[s] * stride
bool nn_gather_normals(const uint8_t* base, uint64_t stride, bool is_f32, const uint32_t* order, uint32_t nf, double* nx, double* ny, double* nz, hipStream_t stream);
size_t nn_plane_partials_bytes(uint64_t n);
bool nn_plane_sums(const Positions& pos, const NnTransform& t, const uint32_t* at, const double* xs, const double* ys, const double* zs, const double* nx,
                   const double* ny, const double* nz, const double origin[3], void* partials, NnPlaneSums* rec, hipStream_t stream);

// M3C2 change detection (m3c2.hip; the argument checks, the scratch and the order of the launches are in m3c2_api.cpp).  The seams
// (pst_m3c2_kernel_shape):
constexpr uint32_t kM3c2LanesPerCore = 64;   // lanes that share one core point: ONE wave searches the rows of its cylinder and tests the candidates
constexpr uint32_t kM3c2CoresPerBlock = 4;   // core points one workgroup of 256 threads owns, one per wave
// one indexed cloud as the cylinder walk reads it (the arrays of a pst_nn_index; nf == 0: nothing is read)
struct M3c2Cloud { const unsigned long long* keys; const double *xs, *ys, *zs; uint32_t nf; NnGrid g; };
struct M3c2Args {
  const uint8_t* core_base; uint64_t core_stride; uint32_t n;
  const uint32_t* order;                // core point of sorted position s (null: s itself)
  const double* normals;                // f64 [n][3] in core order, or null: nx / ny / nz [at[i]]
  const uint32_t* at;                   // per core point the position of its nearest reference point in the index's sorted arrays (0xFFFFFFFF: none)
  const double *nx, *ny, *nz;
  M3c2Cloud cloud[2];                   // reference, compared
  double radius, max_depth, radius2, registration_error;
  uint32_t min_points, flags;
  double* distance; double* lod; uint8_t* significant; uint32_t* counts; double* sums; double* unit_normals;  // each optional
  unsigned long long* n_significant;    // one counter, zeroed by the launcher
  unsigned long long* work;             // three counters (rows searched, candidates tested, members), zeroed by the launcher; null: not counted
};
bool m3c2_run(const M3c2Args& a, hipStream_t stream);

// Height above ground from the k nearest ground points in the XY plane (hag.hip; the grid is sized in hag_grid.hpp, the scratch and the order
// of the launches are in hag_api.cpp).  The seams (pst_hag_kernel_shape):
constexpr uint32_t kHagQueriesPerBlock = 64;       // queries one workgroup of the search kernel owns: ONE wave, one lane per query
constexpr uint32_t kHagMaxK = 32;                  // the k-best list lives in LDS, 16 bytes per slot and lane: 32 KiB per workgroup at the most
constexpr uint32_t kHagBoundsPointsPerBlock = 4096;  // ground points per block partial of the masked bounds, sixteen per lane
// the device-side record of the masked 2-D bounds: the AABB of G in x and y, |G|
struct HagBounds { double min_x, min_y, max_x, max_y; unsigned long long count; };
size_t hag_bounds_partials_bytes(uint64_t n_ground_points);
// G = the points whose three components are finite and whose mask byte is not zero (mask == nullptr: every finite point).  Block partials,
// then one workgroup folds them into *rec; no atomics.  An empty G leaves {+inf, +inf, -inf, -inf, 0}.
bool hag_bounds(const Positions& ground, const uint8_t* mask, void* partials, HagBounds* rec, hipStream_t stream);
// keys[i] = (cy << bits[0]) | cx of ground point i, with bit bits[0] + bits[1] set when i is not in G
bool hag_ground_keys(const Positions& ground, const uint8_t* mask, const HagGrid& g, uint32_t* keys, hipStream_t stream);
// (the positions of G in sorted order: nn_gather; the directory: directory_heads, below)
// keys[i] = the key of query i's cell after its x and y were clamped into the grid's AABB; bit bits[0] + bits[1] alone: not finite.  vals[i] = i
bool hag_query_keys(const Positions& query, const HagGrid& g, uint32_t* keys, uint32_t* vals, hipStream_t stream);
// The search.  query_keys / query_order: the sorted pairs.  hag[i] = q.z - zg, ground_z[i] = zg (each optional); *unresolved += the finite
// queries without a neighbour.  k <= kHagMaxK.
bool hag_search(const Positions& query, const HagGrid& g, uint32_t k, double m2, const uint32_t* query_keys, const uint32_t* query_order, const uint32_t* dir,
                const double* xs, const double* ys, const double* zs, const uint32_t* ground_index, double* hag, double* ground_z, unsigned long long* unresolved,
                hipStream_t stream);
// no ground at all: NaN into both outputs, *unresolved += the finite queries
bool hag_fill_unresolved(const Positions& query, double* hag, double* ground_z, unsigned long long* unresolved, hipStream_t stream);
// mask[i] = 1 iff the byte at addr + i * stride equals value, i < n
bool u8_equals_mask(uint64_t addr, uint64_t stride, uint64_t n, uint8_t value, uint8_t* mask, hipStream_t stream);

// Rasterisation: per-cell statistics of a cloud on an XY grid, and the hole filler (raster.hip; the checks, the grid, the scratch and the order
// of the launches are in raster_api.cpp).  The seams (pst_raster_kernel_shape):
constexpr uint32_t kRasterPointsPerBlock = 1024;  // points per workgroup of the atomic pass, four per lane
constexpr uint32_t kRasterChunk = 256;            // members per chunk of the chunked sums: part of the DEFINITION (include/pasture_amd.h)
constexpr uint32_t kRasterFillMaxHalfWidth = 16;  // the fill's LDS tile is (kPmfTileRows + 2 h) x (kPmfTileCols + 2 h) doubles: 64 x 96 x 8 = 48 KiB at 16
constexpr uint32_t kRasterHeavyBlocks = 1024;     // workgroups of the heavy-cell pass at the most; each takes every kRasterHeavyBlocks-th listed cell
enum : uint32_t { RS_COUNT = 1, RS_MIN = 2, RS_MAX = 4, RS_MEAN = 8, RS_VARIANCE = 16 };
// what a point's value is and which points take part: values == nullptr: z; mask == nullptr: every point
struct RasterInput { const double* values; const uint8_t* mask; };
// the output planes in device memory, rows x cols doubles each; nullptr: not asked for
struct RasterPlanes { double *count, *min, *max, *mean, *variance; };
// every plane's empty-cell value (COUNT +0.0, the others the canonical NaN)
bool raster_fill_empty(const RasterPlanes& out, uint64_t n_cells, hipStream_t stream);
// The atomic path.  min_keys (every byte 0xFF on entry), max_keys, counts (both zeroed): one per cell, each needed only with its plane;
// *members (zeroed) += the members, one integer atomic per workgroup
bool raster_atomic(const Positions& pos, const RasterInput& in, const PmfGrid& g, unsigned long long* min_keys, unsigned long long* max_keys, uint32_t* counts,
                   unsigned long long* members, hipStream_t stream);
bool raster_atomic_decode(const unsigned long long* min_keys, const unsigned long long* max_keys, const uint32_t* counts, uint64_t n_cells, const RasterPlanes& out,
                          hipStream_t stream);
// The sorted path.  keys[i] = row * cols + col of a member, nonmember_key (a power of two not below cols * rows) of every other point
bool raster_keys(const Positions& pos, const RasterInput& in, const PmfGrid& g, uint32_t nonmember_key, uint32_t* keys, hipStream_t stream);
// The heads of every dense directory (dense_directory.hpp drives it).  dir: groups + 1 entries, every byte 0xFF on entry; n >= 1 sorted keys.
// The group of a key is (key >> bx) * cols + its low bx bits: the key itself with bx = 0, cols = 1 (a label, a row-major cell), the cell
// cy * cols + cx of a HagGrid's packed (cy << bx) | cx.  A key whose group is `groups` or more is no member, and the members come first.
// dir[group] = first sorted position of every occupied group, dir[groups] = the first position that holds no member (n: every entry is one);
// pstk::suffix_min_u32 over all of it then makes dir[g] the first sorted position whose group is g or later
bool directory_heads(const uint32_t* sorted_keys, uint32_t n, uint32_t bx, uint32_t cols, uint32_t groups, uint32_t* dir, hipStream_t stream);
// sorted_values[s] = the value of point order[s], s < dir[n_cells]
bool raster_gather(const Positions& pos, const RasterInput& in, const uint32_t* order, const uint32_t* dir, uint32_t n_cells, double* sorted_values, hipStream_t stream);
// One lane per cell walks its segment of sorted_values; a cell of more than kRasterChunk members is appended to heavy_list (*heavy_count,
// zeroed) instead and taken by raster_reduce_heavy, a workgroup per cell; partials: raster_partials_bytes(n) of scratch
size_t raster_partials_bytes(uint64_t n);
bool raster_reduce(const double* sorted_values, const uint32_t* dir, uint32_t n_cells, uint32_t stats, const RasterPlanes& out, uint32_t* heavy_list,
                   uint32_t* heavy_count, hipStream_t stream);
bool raster_reduce_heavy(const double* sorted_values, const uint32_t* dir, uint32_t n, uint32_t n_cells, uint32_t stats, const RasterPlanes& out, const uint32_t* heavy_list,
                         const uint32_t* heavy_count, double* partials, hipStream_t stream);
// The hole filler, out of place: entries that are not finite become the inverse-squared-distance weighted mean of the finite entries of the
// square of h cells around them (the canonical NaN without one); h <= kRasterFillMaxHalfWidth
bool raster_grid_fill(const double* in, double* out, uint32_t cols, uint32_t rows, uint32_t h, hipStream_t stream);

// Minimum-distance (Poisson-disk) subsampling (sample.hip; the checks, the scratch and the loop of rounds are in sample_api.cpp; the index is
// cluster_index.hpp's).  The seams (pst_sample_kernel_shape):
constexpr uint32_t kSamplePointsPerBlock = 256;         // active points one workgroup of the decision kernel owns, one lane each
constexpr uint32_t kSampleSweepsPerLaunch = 2;          // times a lane looks at its point in one launch before it leaves it undecided
constexpr uint32_t kSampleBoundsPointsPerBlock = 4096;  // points per block partial of the bounds, sixteen per lane
// the device-side record of the bounds: the AABB of the finite points and their number ({+inf .., -inf .., 0} without one)
struct SampleBounds { double min[3], max[3]; unsigned long long count; };
size_t sample_bounds_partials_bytes(uint64_t n);
// block partials, then one workgroup folds them into *rec; no atomics
bool sample_bounds(const Positions& pos, void* partials, SampleBounds* rec, hipStream_t stream);
// One launch of the decision kernel over the m active points (active == nullptr: the sorted points 0 .. m - 1, m == nf).  state: one byte per
// sorted point, 0 undecided (what the caller sets before the first round), 1 kept, 2 rejected.  flags: m + 1 entries, flags[t] = 1 iff active
// point t is still undecided afterwards, flags[m] = 0.  shuffled != 0: priority key splitmix64(seed ^ index), else the index.
bool sample_decide(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint32_t* order, uint32_t nf, const ClusterGrid& g,
                   double r2, uint32_t shuffled, uint64_t seed, const uint32_t* active, uint32_t m, uint8_t* state, uint32_t* flags, hipStream_t stream);
// offsets = exclusive sum of flags: next[offsets[t]] = active point t for every flagged t
bool sample_compact(const uint32_t* active, const uint32_t* flags, const unsigned long long* offsets, uint32_t m, uint32_t* next, hipStream_t stream);
// mask[order[s]] = 1 iff s < nf and state[s] is "kept", else 0, for all n sorted positions; *kept (zeroed) += the ones, one integer atomic per workgroup
bool sample_mask(const uint32_t* order, const uint8_t* state, uint64_t n, uint32_t nf, uint8_t* mask, unsigned long long* kept, hipStream_t stream);

// DBSCAN (dbscan.hip; the checks, the scratch and the order of the launches are in dbscan_api.cpp; the index is
// cluster_index.hpp's).  The seam (pst_dbscan_kernel_shape):
constexpr uint32_t kDbscanPointsPerBlock = 256;  // points one workgroup of the count, link and border kernels owns, one lane each
// core[s] = 1 iff sorted point s has at least min_points neighbours, itself included (1 <= min_points <= nf); parent[s] = s; *n_core (zeroed) +=
// the core points, one integer atomic per wave
bool dbscan_count(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, uint32_t nf, const ClusterGrid& g, double e2,
                  uint32_t min_points, uint8_t* core, uint32_t* parent, unsigned long long* n_core, hipStream_t stream);
// the cluster traversal over the core points alone: unite(s, c) for core neighbours s > c
bool dbscan_link(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint8_t* core, uint32_t nf, const ClusterGrid& g,
                 double e2, uint32_t* parent, hipStream_t stream);
// behind dbscan_link: root[s] = the root of a core point / of the core neighbour of smallest (d2, buffer index) / 0xFFFFFFFF for noise; points
// per root and the smallest buffer index per root (both set up here).  The numbering from there is the clusters' (cluster_flag_kept ..
// cluster_ranks above, a filter that keeps everything).
bool dbscan_border(const unsigned long long* sorted_keys, const double* xs, const double* ys, const double* zs, const uint8_t* core, const uint32_t* order, uint32_t nf,
                   const ClusterGrid& g, double e2, uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream);
// behind cluster_ranks: labels[order[s]] = rank of root[s], 0xFFFFFFFF without one; core_out[order[s]] = core[s], 0 for the non-finite points
// (core_out nullable)
bool dbscan_labels(const uint32_t* order, const uint32_t* root, const uint32_t* rank_of_root, const uint8_t* core, uint64_t n, uint32_t nf, uint32_t* labels,
                   uint8_t* core_out, hipStream_t stream);

// Region growing over neighbour lists (region.hip; the checks, the scratch and the order of the launches are in region_api.cpp).  The seams
// (pst_region_kernel_shape):
constexpr uint32_t kRegionThreads = 256;            // threads of one workgroup of the link kernel; classify and attach: one lane per point
uint32_t region_points_per_block(uint32_t k);       // points whose whole lists one workgroup of the link kernel owns: 256, 128, 64 or 32
// state[i] = 0 (a normal component is not finite), 1 (rim) or 2 (smooth: valid and curvature[i] <= curvature_threshold; curvature nullable:
// every valid point); parent[i] = i; *n_smooth (zeroed) += the smooth points, one integer atomic per wave
bool region_classify(const double* normals, const double* curvature, double curvature_threshold, uint32_t n, uint8_t* state, uint32_t* parent, unsigned long long* n_smooth,
                     hipStream_t stream);
// unite(i, j) for every counting slot j of a smooth i that names a smooth point whose normal agrees; knn: uint32 [n][k], 1 <= k <= 64
bool region_link(const Positions& pos, uint32_t k, const uint32_t* knn, const double* normals, const uint8_t* state, double min_abs_cos, double max_distance,
                 uint32_t* parent, hipStream_t stream);
// behind region_link: root[i] = the root of a smooth point / of the first agreeing smooth slot of a rim point / 0xFFFFFFFF; points per root
// and the smallest index per root (both set up here).  The numbering from there is the clusters' (cluster_flag_kept .. cluster_ranks above,
// ids = buffer indices).
bool region_attach(const Positions& pos, uint32_t k, const uint32_t* knn, const double* normals, const uint8_t* state, double min_abs_cos, double max_distance,
                   uint32_t* parent, uint32_t* root, uint32_t* size, uint32_t* min_index, hipStream_t stream);
// behind cluster_ranks: labels[i] = rank of root[i], 0xFFFFFFFF without a kept one; smooth_out[i] = 1 iff state[i] == 2 (smooth_out nullable)
bool region_labels(const uint32_t* root, const uint32_t* rank_of_root, const uint8_t* state, uint32_t n, uint32_t* labels, uint8_t* smooth_out, hipStream_t stream);

// Gather by index and the keys of the device sort orders (reorder.hip; the checks, the scratch and the order of the launches are in
// reorder_api.cpp).  The seams (pst_reorder_kernel_shape):
constexpr uint32_t kReorderPointsPerBlock = 256;      // consecutive OUTPUT points one workgroup owns: one index per lane, read once
constexpr uint32_t kReorderRecordTileBytes = 32768;   // LDS record tile of the paths with an interleaved side, slack included
constexpr uint32_t kReorderTileSlack = 48;            // 16 bytes of target misalignment in front, 32 behind (lds_load reads past a value)
constexpr uint32_t kReorderMinTileRecords = 16;       // records with fewer than this many per tile take the byte-copy kernel
constexpr int kReorderMaxAttrs = 48;                  // attributes per launch; layouts with more are gathered in several launches
// one attribute of a gather: src = address of the attribute of source point 0, dst = of target point dst_first; offset = in the record
struct GatherAttr { uint64_t src, dst; uint32_t src_stride, dst_stride, offset, size; };
struct GatherArgs {
  const void* idx;              // count indices, u32 or u64 (idx64), device memory
  uint64_t count, src_len;
  uint64_t src_rec, dst_rec;    // interleaved sides: address of source record 0 / of target record dst_first
  uint32_t idx64, stride;       // stride: the record size (both layouts are equal)
  uint32_t chunk;               // records per pass over the LDS record tile
  uint32_t n_attrs;
  uint32_t dst_covered;         // the attributes cover every byte of a record: a tile without skipped points need not be read first
  uint32_t count_skipped;       // add the out-of-range entries to *skipped (one launch of a call does)
  unsigned long long* skipped;  // nullable
  GatherAttr attrs[kReorderMaxAttrs];
};
uint32_t gather_chunk(uint32_t stride);      // records per LDS tile pass; below kReorderMinTileRecords: gather_tile_fits is false
bool gather_tile_fits(uint32_t stride);
// dst[dst_first + j] = src[idx[j]], j < count; an index >= src_len leaves its target point alone and is counted.  by_bytes: the plain
// per-attribute byte-copy kernel (any record size).  Interleaved to interleaved in the tile kernel moves whole records (a.attrs unused).
bool gather_points(const GatherArgs& a, bool src_aos, bool dst_aos, bool by_bytes, hipStream_t stream);
// out2[0] = max index, out2[1] = entries >= src_len (both zeroed by the caller)
bool gather_index_check(const void* idx, bool idx64, uint64_t count, uint64_t src_len, unsigned long long* out2, hipStream_t stream);
// Sort keys of one component of a numeric attribute (the value of point i at addr + i * stride; ct: its component type): ascending key order
// is np.argsort(values, kind="stable") with NaNs last; descending complements every key that is not a NaN key.  keys32 for types of up to
// 32 bits, else keys64 and vals[i] = i.
bool reorder_attribute_keys(uint64_t addr, uint64_t stride, uint64_t n, uint32_t ct, bool descending, uint32_t* keys32, unsigned long long* keys64, uint32_t* vals,
                            hipStream_t stream);
// cell = clamp(floor((p - min) * inv)) per axis, `bits` bits each, interleaved x lowest; dims 2 (x, y) or 3
struct MortonGrid { double min[3], inv[3]; uint32_t dims, bits; };
// sort_keys[i]: the Morton key, bit dims * bits set alone for a point with a coordinate that is not finite; vals[i] = i; out_keys (nullable):
// the same with 1 << 63 for those points
bool reorder_morton_keys(const Positions& pos, const MortonGrid& g, unsigned long long* sort_keys, uint32_t* vals, unsigned long long* out_keys, hipStream_t stream);
// keys[i] = splitmix64(seed ^ i), vals[i] = i
bool reorder_shuffle_keys(uint64_t n, uint64_t seed, unsigned long long* keys, uint32_t* vals, hipStream_t stream);
// inverse[order[j]] = j for every order[j] < n
bool reorder_invert(const uint32_t* order, uint64_t n, uint32_t* inverse, hipStream_t stream);

// Point-in-polygon ids and masks (crop.hip; the checks and the set's device memory are in crop_api.cpp, the index in polygon_index.hpp).  The
// seams (pst_crop_kernel_shape):
constexpr uint32_t kCropFlatPointsPerBlock = 1024;   // points one workgroup of the flat body serves from its LDS copy of the entries, four per lane
constexpr uint32_t kCropBandedPointsPerBlock = 256;  // points per workgroup of the banded body, one lane each
// Entries up to which the automatic choice takes the flat body.  Set by the LDS capacity -- 36 bytes per entry (the record and its polygon
// index) make 36 KiB, four workgroups per compute unit of its 160 KiB -- because the measurement found no crossover below it: at 4, 64, 512
// and 1024 entries on 10^8 points the flat body took 0.34 - 0.44 of the banded body's time (profiles/crop_1e8.json).
constexpr uint32_t kCropFlatMaxEdges = 1024;
constexpr uint32_t kCropNoPolygon = 0xFFFFFFFFu;
// A set in device memory.  records: 4 doubles {lo.x, lo.y, hi.x, hi.y} each, 32-byte aligned; polygon: the polygon index of every record.
// Flat: the n_records entries, sorted by polygon.  Banded: the band lists one after the other, list b = records offsets[b] .. offsets[b + 1],
// each sorted by polygon; ymin, scale, bands: pst::polygon::Bands.
struct CropSet {
  const double* records;
  const uint32_t* polygon;
  const uint32_t* offsets;
  uint32_t n_records, bands;
  double xmin, ymin, xmax, ymax, scale;
};
// One launch.  ids (nullable): the smallest polygon index that contains point i, kCropNoPolygon without one.  mask (nullable): 1 iff
// (id != kCropNoPolygon) != (outside != 0).  *count (nullable, zeroed by the caller) += the ones of the mask -- without a mask the ids that
// name a polygon -- one integer atomic per wave.  flat needs n_records <= kCropFlatMaxEdges.
bool crop_query(const Positions& pos, const CropSet& set, bool flat, uint32_t* ids, uint8_t* mask, int outside, unsigned long long* count, hipStream_t stream);
// the byte at addr + i * stride = values[ids[i]] wherever ids[i] < n_values, i < n; *written (nullable, zeroed by the caller) += those points
bool set_u8_from_ids(uint64_t addr, uint64_t stride, uint64_t n, const uint32_t* ids, const uint8_t* values, uint32_t n_values, unsigned long long* written,
                     hipStream_t stream);

// Individual trees: the local-maximum filter and the crowns (trees.hip; the window in trees_window.hpp; the checks, the scratch and the order
// of the launches in trees_api.cpp).  The index is the dense 2-D grid's (dense_grid_device.hpp, dense_directory.hpp) over the members a
// byte selects, with the height of every member next to its x and y.  The seams (pst_trees_kernel_shape):
constexpr uint32_t kTreesPointsPerBlock = 256;         // candidates one workgroup of the near pass owns, one lane each
constexpr uint32_t kTreesSurvivorsPerBlock = 4;        // survivors one workgroup of the far pass owns, ONE wave each
constexpr uint32_t kTreesQueriesPerBlock = 64;         // queries one workgroup of the crown search owns: one wave, one lane per query
constexpr uint32_t kTreesBoundsPointsPerBlock = 4096;  // points per block partial of the member pass, sixteen per lane
// what a point's height is and which points take part: heights == nullptr: z; mask == nullptr: every point
struct TreesInput { Positions pos; const double* heights; const uint8_t* mask; };
// the device-side record of the member pass: the AABB of the members in x and y, the largest |h| among them, their number
struct TreesBounds { double min_x, min_y, max_x, max_y, max_abs_h; unsigned long long count; };
size_t trees_bounds_partials_bytes(uint64_t n);
// member[i] = 1 iff x, y and h of point i are finite, both masks (in.mask, also; each nullable) are not zero there and h >= floor (-inf:
// every valid point), else 0; block partials of the members' bounds, then one workgroup folds them into *rec; no atomics
bool trees_members(const TreesInput& in, const uint8_t* also, double floor, uint8_t* member, void* partials, TreesBounds* rec, hipStream_t stream);
// keys[e] = (cy << bits[0]) | cx of point i = subset ? subset[e] : e, with bit bits[0] + bits[1] set when member (nullable) is 0 there; e < count
bool trees_keys(const Positions& pos, const uint32_t* subset, const uint8_t* member, uint64_t count, const HagGrid& g, uint32_t* keys, hipStream_t stream);
// x, y, h and the buffer index (index, nullable) of point i = subset ? subset[order[s]] : order[s] for the m sorted positions s
bool trees_gather(const TreesInput& in, const uint32_t* subset, const uint32_t* order, uint32_t m, double* xs, double* ys, double* hs, uint32_t* index, hipStream_t stream);
// The near pass over the nc sorted candidates: the 3 x 3 cells around a candidate, clipped to its window's box.  A dominator there decides
// it (no top); none and a box inside those cells decides it too (top_mask[index[s]] = 1); flags[s] = 1 for the others, flags[nc] = 0.
bool trees_filter_near(const TreeWindow& w, const HagGrid& g, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index, uint32_t nc,
                       uint8_t* top_mask, uint32_t* flags, hipStream_t stream);
// The far pass over the m listed survivors, a wave each: every row of the window's box, its candidates across the lanes, until a dominator
// is seen.  work (nullable, zeroed by the caller): += candidates tested.
bool trees_filter_far(const TreeWindow& w, const HagGrid& g, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index,
                      const uint32_t* survivors, uint32_t m, uint8_t* top_mask, unsigned long long* work, hipStream_t stream);
// flags[i] = bytes[i] != 0 for i < n, flags[n] = 0
bool trees_flags(const uint8_t* bytes, uint64_t n, uint32_t* flags, hipStream_t stream);
// offsets = exclusive sum of flags: list[offsets[i]] = i and keys[offsets[i]] = the order-REVERSING image of h_i (of h_i + 0.0: the two
// zeros get one key) for every flagged i
bool trees_list(const TreesInput& in, const uint32_t* flags, const unsigned long long* offsets, uint64_t n, unsigned long long* keys, uint32_t* list, hipStream_t stream);
// keys[i] = the key of point i's cell after its x and y were clamped into the grid's AABB, for a valid point (as trees_members) with
// h >= floor; bit bits[0] + bits[1] alone for every other point.  vals[i] = i
bool trees_query_keys(const TreesInput& in, double floor, const HagGrid& g, uint32_t* keys, uint32_t* vals, hipStream_t stream);
// The crown search over the sorted queries: the top of smallest (d2, buffer index) within m2, by dense_grid_device.hpp's ring walk with k = 1;
// then ids[i] = number[at] iff d2 <= rc*rc && h >= exclusion*H, rc = half_factor*H, H = hs[at], else 0xFFFFFFFF (and for every point that is
// no query).  counts[t] (nt zeroed entries) += the points labelled t, *labelled (zeroed) += all of them, folded per wave.
bool trees_crown_search(const TreesInput& in, uint32_t n, const HagGrid& g, double m2, double half_factor, double exclusion, const uint32_t* query_keys,
                        const uint32_t* query_order, const uint32_t* dir, const double* xs, const double* ys, const double* hs, const uint32_t* index,
                        const uint32_t* number, uint32_t* ids, uint32_t* counts, unsigned long long* labelled, hipStream_t stream);

// Segment statistics: per-label count, box, centroid, covariance and value statistics (segments.hip; the checks, the scratch and the order of
// the launches are in segments_api.cpp).  The directory is dense_directory.hpp's.  The seams
// (pst_segments_kernel_shape):
constexpr uint32_t kSegmentsPointsPerBlock = 256;  // points one workgroup of the key and gather kernels owns, one lane each
constexpr uint32_t kSegmentGroup = 256;            // elements one wave folds: part of the DEFINITION (PST_SEGMENT_GROUP, include/pasture_amd.h)
constexpr uint32_t kSegmentsGroupsPerBlock = 4;    // groups per workgroup of the fold kernel, ONE wave each
enum : uint32_t { SG_COUNT = 1, SG_BOUNDS = 2, SG_CENTROID = 4, SG_COVARIANCE = 8, SG_VALUE_MIN = 16, SG_VALUE_MAX = 32, SG_VALUE_MEAN = 64, SG_VALUE_VARIANCE = 128 };
// labels: one per point; values == nullptr: z; mask == nullptr: every point
struct SegmentInput { const uint32_t* labels; const double* values; const uint8_t* mask; };
// the output planes in device memory, S doubles per plane: count 1, min 3, max 3, centroid 3, covariance 6, the value's four 1 each; nullptr: not asked for
struct SegmentPlanes { double *count, *min, *max, *centroid, *covariance, *value_min, *value_max, *value_mean, *value_variance; };
// keys[i] = the label of a member, n_segments of every other point
bool segment_keys(const Positions& pos, const SegmentInput& in, uint32_t n_segments, uint32_t* keys, hipStream_t stream);
// x, y, z and the value (vs nullable: no values, the value is z) of point order[s] for the sorted positions s < dir[n_segments]
bool segment_gather(const Positions& pos, const SegmentInput& in, const uint32_t* order, const uint32_t* dir, uint32_t n_segments, double* xs, double* ys, double* zs,
                    double* vs, hipStream_t stream);
// count[s] = members of s, groups[s] = ceil(count / 256), entry n_segments of both 0; the COUNT plane, and every other plane and the apex
// (nullable) of a segment without members
bool segment_counts(const uint32_t* dir, uint32_t n_segments, const SegmentPlanes& out, uint32_t* apex, uint32_t* count, uint32_t* groups, hipStream_t stream);
// next_count[s] = groups[s] where that is more than one, else 0 (the segment is finished); next_groups = ceil(next_count / 256); n_segments + 1 entries
bool segment_next_level(const uint32_t* groups, uint32_t n_segments, uint32_t* next_count, uint32_t* next_groups, hipStream_t stream);
// One level of the fold.  count[s] elements of segment s start at element_offset[s] of every input array; group_offset = the exclusive sum of
// ceil(count / 256) (n_segments + 1 entries, the last n_groups); partial_offset = the next level's element_offset, where a segment of more
// than one group writes its partials.
struct SegmentLevel { uint64_t n_groups; const unsigned long long *group_offset, *element_offset, *partial_offset; const uint32_t* count; };
// A channel with a null input is not computed.  A segment of one group writes result[s] -- a sum divided by (double) of its members
// (dir[s + 1] - dir[s]) --, every other its partials to `out`.  Sums: up to seven channels.  Minima and maxima: x y z v, read through the
// ordered key; apex_in rides with max channel 3 (the lowest apex_in among the elements of the largest key).  results are nullable.
// products: sum_in is not read; the elements of sums 0 .. 5 are the products xx xy xz yy yz zz of column[0 .. 2] - mean[0 .. 2][s], those of
// sum 6 the square of column[3] - mean[3][s], for the sums whose result is not null (minima and maxima are not computed).
struct SegmentFold {
  SegmentLevel level;
  const uint32_t* dir;
  uint32_t n_segments;
  const double* sum_in[7]; double* sum_out[7]; double* sum_result[7];
  const double* min_in[4]; double* min_out[4]; double* min_result[4];
  const double* max_in[4]; double* max_out[4]; double* max_result[4];
  const uint32_t* apex_in; uint32_t* apex_out; uint32_t* apex_result;
  const double* column[4]; const double* mean[4];
};
bool segment_fold(const SegmentFold& f, bool products, hipStream_t stream);

// Group order statistics: quantiles and counts above a threshold per cell or per segment (quantiles.hip; the checks, the scratch and the order
// of the launches are in quantiles_api.cpp).  Keys and gather are raster.hip's and segments.hip's, the directory dense_directory.hpp's.  The seams
// (pst_quantiles_kernel_shape):
constexpr uint32_t kQuantilesPointsPerBlock = 1536;  // sorted positions whose groups one workgroup of the window kernel owns
constexpr uint32_t kQuantilesCap = 512;              // the largest group the window kernel sorts in LDS; a larger one is listed
constexpr uint32_t kQuantilesWindow = 2048;          // sorted positions one workgroup loads and sorts: >= points per block + cap - 1
enum : uint32_t { QM_LINEAR = 0, QM_LOWER = 1, QM_HIGHER = 2 };
// param: the probabilities, then the thresholds.  The output is out[1 + n_probs + n_thresholds][n_groups], plane 0 the COUNT
struct QuantileRequest { double param[64]; uint32_t n_probs, n_thresholds, method; };
// heavy_list and heavy_size: this many entries and one more
size_t quantile_heavy_capacity(uint64_t n, uint64_t n_groups, uint32_t cap);
// One lane per group: the COUNT plane; an empty group's planes (the canonical NaN, +0.0); a group of more than `cap` members is appended to
// heavy_list with its size in heavy_size (*heavy_count, zeroed)
bool quantile_groups(const uint32_t* dir, uint32_t n_groups, uint32_t cap, const QuantileRequest& rq, double* out, uint32_t* heavy_list, uint32_t* heavy_size,
                     uint32_t* heavy_count, hipStream_t stream);
// The planes of every group of 1 .. cap members (cap <= kQuantilesCap; 0: nothing to do).  sorted_keys[s] = the group of sorted position s
// for s < dir[n_groups]; n = the length of both arrays
bool quantile_small_groups(const double* sorted_values, const uint32_t* sorted_keys, const uint32_t* dir, uint32_t n, uint32_t n_groups, uint32_t cap,
                           const QuantileRequest& rq, double* out, hipStream_t stream);
// The listed groups, `heavy` of them, with heavy_offset = the exclusive sum of heavy_size (heavy + 1 entries, the last n_listed): the listed
// members' keys, slots[j] = j and owner[j] = the place of j's group in the list
bool quantile_heavy_compact(const double* sorted_values, const uint32_t* dir, const uint32_t* heavy_list, const unsigned long long* heavy_offset, uint32_t heavy,
                            uint32_t n_listed, unsigned long long* keys, uint32_t* slots, uint32_t* owner, hipStream_t stream);
// keys[r] = owner[slots[r]]
bool quantile_owner_gather(const uint32_t* owner, const uint32_t* slots, uint32_t n, uint32_t* keys, hipStream_t stream);
// ranked: the slots ordered by (owner, key).  One wave per listed group writes its planes
bool quantile_heavy_select(const double* sorted_values, const uint32_t* dir, uint32_t n_groups, const uint32_t* heavy_list, const unsigned long long* heavy_offset,
                           uint32_t heavy, const uint32_t* ranked, const QuantileRequest& rq, double* out, hipStream_t stream);

// Fixed-radius neighbour search over a pst_nn_index (radius.hip; the checks, the scratch and the order of the launches are in
// radius_api.cpp).  Query keys and their sort are nn.hip's.  The seams (pst_radius_kernel_shape):
constexpr uint32_t kRadiusQueriesPerBlock = 256;          // queries one workgroup of the count and fill kernels owns, one lane each
constexpr uint32_t kRadiusSortCap = 512;                  // the longest list the window kernel orders in LDS; a longer one is listed
constexpr uint32_t kRadiusSortWindow = 2048;              // entries one workgroup loads and sorts: >= positions per block + cap - 1
constexpr uint32_t kRadiusSortPositionsPerBlock = 1536;   // entry positions whose lists one workgroup of the window kernel owns
// The queries in the order of their cell keys (query_keys, query_order: nn_query_keys and the pair sort), the index's sorted arrays.
struct RadiusSearch {
  Positions pos; NnTransform t; NnGrid g; double radius, r2;
  const unsigned long long* query_keys; const uint32_t* query_order;
  const unsigned long long* keys; const double *xs, *ys, *zs; const uint32_t* target_index; uint32_t nf;
};
// counts[i] = the neighbours of query i (buffer order), every query
bool radius_count(const RadiusSearch& a, uint32_t* counts, hipStream_t stream);
// the same walk: query i writes the buffer index and the ordered key of d2 of its neighbours into [offsets[i], offsets[i + 1]), in walk order
bool radius_fill(const RadiusSearch& a, const unsigned long long* offsets, uint32_t* indices, unsigned long long* d2_keys, hipStream_t stream);
// Every list of 1 .. cap entries (cap <= kRadiusSortCap; 0: nothing to do) ordered by (d2 key, index) in place; distances (nullable) = sqrt(d2)
bool radius_order_short(const unsigned long long* offsets, uint32_t n, uint64_t total, uint32_t cap, uint32_t* indices, const unsigned long long* d2_keys, double* distances,
                        hipStream_t stream);
// the lists of more than cap entries appended to long_list with their lengths in long_size (*long_count, zeroed)
bool radius_list_long(const unsigned long long* offsets, uint32_t n, uint32_t cap, uint32_t* long_list, uint32_t* long_size, uint32_t* long_count, hipStream_t stream);
// The listed lists, `n_long` of them, with long_offset = the exclusive sum of long_size (n_long + 1 entries, the last n_listed): the listed
// entries' indices (twice: one copy is the first sort's input), d2 keys and owner[j] = the place of j's list in long_list
bool radius_long_compact(const unsigned long long* offsets, const uint32_t* long_list, const unsigned long long* long_offset, uint32_t n_long, uint32_t n_listed,
                         const uint32_t* indices, const unsigned long long* d2_keys, uint32_t* idx, uint32_t* idx_keys, unsigned long long* keys, uint32_t* owner,
                         hipStream_t stream);
// out[r] = keys[slots[r]] (64 bits) and out[r] = owner[slots[r]] (32 bits)
bool radius_gather_u64(const unsigned long long* keys, const uint32_t* slots, uint32_t n, unsigned long long* out, hipStream_t stream);
bool radius_gather_u32(const uint32_t* owner, const uint32_t* slots, uint32_t n, uint32_t* out, hipStream_t stream);
// ranked: the slots ordered by (owner, d2 key, index), sorted_owner: their owners.  Entry r goes to its list's place r - long_offset[owner]
bool radius_long_scatter(const unsigned long long* offsets, const uint32_t* long_list, const unsigned long long* long_offset, uint32_t n_listed, const uint32_t* ranked,
                         const uint32_t* sorted_owner, const uint32_t* idx, const unsigned long long* keys, uint32_t* indices, double* distances, hipStream_t stream);

}  // namespace pstk
