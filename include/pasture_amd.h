/*
 * pasture_amd — C ABI of the MI355X-native implementation of pasture's per-point attribute-transform hot path.
 *
 * The reference (igd-geo/pasture, Rust) has no FFI on this path; its seam is the Rust trait surface
 * (BorrowedBuffer / InterleavedBuffer / ColumnarBuffer / PointLayout) plus the entry points listed below.  Every
 * function here names the reference interface it replaces (paths relative to the reference checkout).  A Rust
 * shim that re-implements those traits on top of this ABI is sketched in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns a pst_status; 0 = ok.  The reference signals precondition violations with
 *    panic!/assert!/expect; nothing unwinds across this ABI — the shim re-raises codes 2..14 as panic!.
 *    pst_last_error() returns the panic message of the last failing call on the calling thread.
 *  - plain pointers and sizes only; no torch / C++ types.  Device pointers are HIP device addresses.
 *  - all device work is enqueued on the calling thread's current stream (pst_set_stream; default = the null
 *    stream).  Functions that return results to host memory synchronise that stream before returning; the
 *    *_async variants do not.
 *  - there is NO CPU fallback: compute entry points fail with PST_ERR_NO_DEVICE / PST_ERR_HIP when no gfx950
 *    device is usable.  Host-only logic (layouts, converter mapping construction, argument checks) works
 *    without a device.
 */
#ifndef PASTURE_AMD_H
#define PASTURE_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pst_status {
  PST_OK = 0,
  PST_ERR_INVALID_ARGUMENT = 1,
  PST_ERR_LAYOUT_MISMATCH = 2,         /* buffer_conversion.rs:302-303 assert_eq! on layouts */
  PST_ERR_RANGE = 3,                   /* buffer_conversion.rs:304-306 range asserts, slice bounds */
  PST_ERR_MISSING_ATTRIBUTE = 4,       /* .expect("... not found in ... PointLayout") */
  PST_ERR_INVALID_CONVERSION = 5,      /* attribute_conversion.rs:267-269 "Invalid conversion X -> Y" */
  PST_ERR_TRANSFORM_TYPE_MISMATCH = 6, /* buffer_conversion.rs:209-213 */
  PST_ERR_UNSUPPORTED_TRANSFORM = 7,   /* closure outside the closed descriptor set: use the CPU path */
  PST_ERR_DUPLICATE_ATTRIBUTE = 8,     /* point_layout.rs:783-788 */
  PST_ERR_INVALID_LAYOUT = 9,          /* point_layout.rs:725-745, Layout::from_size_align failures */
  PST_ERR_BOUNDS_INVALID = 10,         /* math/bounds.rs:21-26 AABB::from_min_max panic (e.g. all-NaN input) */
  PST_ERR_TOO_FEW_POINTS = 11,         /* normal_estimation.rs:86-88 */
  PST_ERR_K_TOO_SMALL = 12,            /* normal_estimation.rs:89-91 */
  PST_ERR_NOT_ENOUGH_NEIGHBOURS = 13,  /* normal_estimation.rs:471 unwrap on Err */
  PST_ERR_UNSUPPORTED_ATTRIBUTE = 14,  /* voxel_grid.rs:475 "Waveform data currently not supported!", :683 non-standard attribute */
  PST_ERR_HIP = 20,
  PST_ERR_NO_DEVICE = 21,
  PST_ERR_OUT_OF_MEMORY = 22,
  PST_ERR_UNSUPPORTED = 23
} pst_status;

/* PointAttributeDataType, point_layout.rs:23-68; kind = declaration order :25-50 */
enum {
  PST_U8 = 0, PST_I8, PST_U16, PST_I16, PST_U32, PST_I32, PST_U64, PST_I64, PST_F32, PST_F64,
  PST_VEC3U8, PST_VEC3U16, PST_VEC3F32, PST_VEC3I32, PST_VEC3F64, PST_VEC4U8, PST_BYTEARRAY, PST_CUSTOM
};
typedef struct pst_datatype {
  uint32_t kind;
  uint32_t reserved;
  uint64_t size_param;  /* ByteArray(length) / Custom.size */
  uint64_t align_param; /* Custom.min_alignment */
  uint8_t uuid[16];     /* Custom.name */
} pst_datatype;

/* PointAttributeMember, point_layout.rs:353-431 */
typedef struct pst_member {
  const char* name; /* borrowed from the layout; valid until the layout is destroyed or mutated */
  pst_datatype datatype;
  uint64_t offset;
  uint64_t size;
} pst_member;

/* Closed set of attribute transformations standing in for the reference's `Fn(T) -> T` closures
 * (buffer_conversion.rs:14-31, :194-234).  Anything else must stay on the CPU path. */
enum { PST_XF_NONE = 0, PST_XF_AFFINE = 1, PST_XF_BITFIELD = 2 };
typedef struct pst_transform {
  uint32_t kind;
  uint32_t shift;        /* BITFIELD: (v >> shift) & mask on U8/U16/U32/U64 — raw_readers.rs:61-164 */
  pst_datatype datatype; /* the closure's T; checked like buffer_conversion.rs:209-213 */
  double scale[3];       /* AFFINE on F64/Vec3f64: (p*scale)+offset, two roundings, never fused — raw_readers.rs:42-48; */
  double offset[3];      /*        on F32/Vec3f32: ((p as f64*scale)+offset) as f32 — raw_readers.rs:49-55            */
  uint64_t mask;
} pst_transform;

typedef struct pst_mapping_info { /* AttributeMapping, buffer_conversion.rs:41-55 (introspection) */
  const char* source_name;
  const char* target_name;
  pst_datatype source_datatype;
  pst_datatype target_datatype;
  uint64_t source_offset;
  uint64_t target_offset;
  int32_t has_converter;
  uint32_t transform_kind;
  int32_t apply_to_source;
  int32_t reserved;
} pst_mapping_info;

typedef struct pst_layout pst_layout;       /* PointLayout,           point_layout.rs:648-997 */
typedef struct pst_buffer pst_buffer;       /* VectorBuffer :659 / HashMapBuffer :1031 / ExternalMemoryBuffer :1479 (point_buffer.rs) */
typedef struct pst_converter pst_converter;
typedef struct pst_point_converter pst_point_converter;
typedef struct pst_comm pst_comm;           /* RCCL communicator(s) of the sharded path */
typedef struct pst_comm_id { uint8_t bytes[128]; } pst_comm_id;  /* rendezvous token (RCCL unique id), shared out of band */ /* BufferLayoutConverter, buffer_conversion.rs:98-663 */

const char* pst_last_error(void);

/* ---- device / stream ------------------------------------------------------------------------------- */
int pst_device_count(int* out);
int pst_set_device(int device);
int pst_set_stream(void* hip_stream); /* hipStream_t; thread-local; NULL = null stream */
int pst_get_stream(void** out_hip_stream); /* the calling thread's current stream (so that a helper can restore it) */
int pst_stream_synchronize(void);
/* Frees the device scratch the calling thread's pst_compute_normals* calls keep between calls, per device (about 55 bytes per point of the
 * largest recent cloud, never more than PST_SCRATCH_MAX_BYTES = 16 GiB by default; the reference's temporaries die with every call: normal_estimation.rs:79-130),
 * and hands the unused blocks of the current device's stream-ordered pool -- the memory of destroyed / shrunk buffers, which the library keeps for its next
 * allocation -- back to the driver, where other allocators of the process (hipMalloc) can get at them.  Synchronises the device.  Never needed for correctness:
 * an allocation of the library that fails for lack of memory does the same and tries once more before it reports PST_ERR_OUT_OF_MEMORY. */
int pst_release_scratch(void);
/* The PST_KNN_* / PST_SCRATCH_MAX_BYTES tuning switches are read from the environment ONCE (first use) -- never on the call path.  This reads them
 * again: for test and A/B harnesses that change them inside one process.  Not to be called while another thread is inside the library. */
int pst_reload_tuning(void);

/* ---- PointLayout ------------------------------------------------------------------------------------ */
int pst_layout_create(pst_layout** out);                           /* PointLayout::default()            :1011-1023 */
int pst_layout_destroy(pst_layout* l);
int pst_layout_clone(const pst_layout* l, pst_layout** out);
/* add_attribute(attr, FieldAlignment::{Default | Packed(max_alignment)})                               :778-822  */
int pst_layout_add_attribute(pst_layout* l, const char* name, const pst_datatype* dt, uint32_t packed, uint64_t max_alignment);
int pst_layout_from_members(const pst_member* members, size_t n, uint64_t type_alignment, pst_layout** out); /* :719-759 */
int pst_layout_num_attributes(const pst_layout* l, size_t* out);
int pst_layout_get_member(const pst_layout* l, size_t index, pst_member* out);                           /* at() :898-900 */
int pst_layout_size_of_point_entry(const pst_layout* l, uint64_t* out);                                  /* :928-931 */
int pst_layout_alignment(const pst_layout* l, uint64_t* out);
int pst_layout_equals(const pst_layout* a, const pst_layout* b, int* out);                                /* derive(PartialEq) :646 */

/* ---- buffers ------------------------------------------------------------------------------------------ */
enum { PST_STORAGE_INTERLEAVED = 0, PST_STORAGE_COLUMNAR = 1 };
enum { PST_MEM_DEVICE = 0, PST_MEM_PINNED_HOST = 1 };
/* MakeBufferFromLayout::new_from_layout (:497-500): empty buffer, library-owned memory of `memkind`.
 * Interleaved: one allocation, stride = size_of_point_entry.  Columnar: one 256-B aligned column per attribute. */
int pst_buffer_create(const pst_layout* l, uint32_t storage, uint32_t memkind, pst_buffer** out);
/* ExternalMemoryBuffer<T: AsRef<[u8]>> (:1479-1708): interleaved view over caller-owned device-accessible memory;
 * len = nbytes / size_of_point_entry; nbytes must be a multiple of the point size (:1488-1497).  Any base address (records behind a file header).
 * "Device-accessible" is checked (both ends of the range, hipPointerGetAttributes): device memory, managed memory, or host memory the device maps
 * (hipHostMalloc / hipHostRegister); ordinary host memory -- what the reference's type wraps -- is PST_ERR_INVALID_ARGUMENT here instead of a GPU fault
 * at the first kernel.  PST_EXTERNAL_UNCHECKED=1 skips the check.  The same holds for every column of pst_buffer_wrap_external_columns. */
int pst_buffer_wrap_external(const pst_layout* l, void* device_ptr, size_t nbytes, pst_buffer** out);
/* Columnar view over caller-owned columns (one device pointer per layout attribute, layout order), `len` points. */
int pst_buffer_wrap_external_columns(const pst_layout* l, void* const* column_ptrs, size_t len, pst_buffer** out);
/* SliceBuffer::slice / SliceBufferMut::slice_mut, pasture-core/src/containers/slice.rs:16-43 (BufferSlice :76-330): a non-owning view of
 * points [first, first + count) of `parent` with the parent's layout and storage kind.  Every entry point that takes a buffer takes a
 * slice: calculate_bounds(&buf.slice(a..b)), the chunked minmax_attribute of pasture-tools/src/bin/info.rs:66-78, transform_attribute on
 * slice_mut, compute_normals, conversions from / into it.  A range outside the parent is PST_ERR_RANGE (the slice's index assertions
 * :52-75); a slice cannot be resized (PST_ERR_UNSUPPORTED: it is not an OwningBuffer).  It borrows the parent's memory: destroy it
 * before the parent is resized or destroyed (what the borrow checker enforces in Rust).  The library checks what the borrow checker would:
 * every owning buffer carries a storage epoch that its resize and destroy bump, and any later use of a slice cut before that (or of a slice
 * of such a slice) is PST_ERR_INVALID_ARGUMENT -- never a read of freed device memory.  (pst_buffer_destroy of the stale slice itself
 * still succeeds.  Slices of caller-owned external memory are not tracked: that memory's lifetime is the caller's.) */
int pst_buffer_slice(const pst_buffer* parent, size_t first, size_t count, pst_buffer** out);
int pst_buffer_destroy(pst_buffer* b);
int pst_buffer_len(const pst_buffer* b, size_t* out);                 /* BorrowedBuffer::len :29 */
int pst_buffer_resize(pst_buffer* b, size_t count);                   /* OwningBuffer::resize :263 — new points zero-filled */
/* BorrowedMutBuffer::swap (point_buffer.rs:229; VectorBuffer :770-783, HashMapBuffer :1276-1292, ExternalMemoryBuffer :1591-1612): exchanges two
 * points in place, on the current stream (three small device copies per record / per column through the library's scratch).  Either index out of
 * bounds -> PST_ERR_RANGE (the reference's assert!); equal indices return at once.  Not a bulk path: a per-point device round trip. */
int pst_buffer_swap(pst_buffer* b, size_t from_index, size_t to_index);
int pst_buffer_is_columnar(const pst_buffer* b, int* out);            /* as_columnar / as_interleaved probes :143-151 */
int pst_buffer_layout(const pst_buffer* b, pst_layout** out_clone);   /* point_layout() :33 (returns a clone) */
int pst_buffer_points_ptr(const pst_buffer* b, void** out);           /* get_point_range_ref(0..len).as_ptr() :524-526 */
int pst_buffer_column_ptr(const pst_buffer* b, const char* name, const pst_datatype* dt, void** out); /* get_attribute_range_ref :593-599 */
/* host <-> buffer transfers (synchronous) */
int pst_buffer_write_points(pst_buffer* b, size_t first, size_t count, const void* host_src);  /* set_point_range :90 */
int pst_buffer_read_points(const pst_buffer* b, size_t first, size_t count, void* host_dst);   /* get_point_range :45 */
int pst_buffer_write_attribute(pst_buffer* b, const char* name, const pst_datatype* dt, size_t first, size_t count, const void* host_src); /* set_attribute_range :110 */
int pst_buffer_read_attribute(const pst_buffer* b, const char* name, const pst_datatype* dt, size_t first, size_t count, void* host_dst);  /* get_attribute_range :71 */
/* view_attribute_with_conversion::<T>(attribute).into_iter().collect(), point_buffer.rs:322-330 / buffer_views.rs:533-650: the attribute `name`
 * of points [first, first + count) converted from its stored datatype to `target_dt` with the Rust-`as` table (convert_unit when they are
 * equal).  Not in the layout -> PST_ERR_MISSING_ATTRIBUTE (:549-552); no conversion between the datatypes -> PST_ERR_INVALID_CONVERSION
 * ("Conversion between attribute types is impossible", :553-561).  _device: the dense array of `target_dt` values lands in device memory,
 * stream-ordered. */
int pst_buffer_read_attribute_converted(const pst_buffer* b, const char* name, const pst_datatype* target_dt, size_t first, size_t count, void* host_dst);
int pst_buffer_read_attribute_converted_device(const pst_buffer* b, const char* name, const pst_datatype* target_dt, size_t first, size_t count, void* device_dst);
/* deterministic synthetic points generated on the device (DESIGN.md "Synthetic inputs") */
int pst_buffer_synth_fill(pst_buffer* b, uint64_t seed, uint64_t first_index);

/* OwningBufferExt::append (point_buffer.rs:419-489): appends every point of `other`; the layouts must be equal
 * (PST_ERR_LAYOUT_MISMATCH = the assert_eq! of :420).  Capacity grows geometrically like Vec. */
int pst_buffer_append(pst_buffer* self, const pst_buffer* other);
/* HashMapBuffer::filter_into (point_buffer.rs:1082-1136): order-preserving compaction of the points whose predicate holds into
 * dst[0, matches).  The predicate `Fn(usize) -> bool` is passed as a byte mask of src->len entries (mask[i] != 0 keeps
 * point i; benches/buffer_filter_bench.rs:62-64); mask_memkind = PST_MEM_DEVICE for a device pointer, anything else = host.
 * num_matches_hint < 0 = None.  Panics of the reference: layouts differ -> PST_ERR_LAYOUT_MISMATCH; dst shorter than
 * num_matches -> PST_ERR_RANGE; more matches than the hint -> PST_ERR_RANGE (slice index out of range).
 * *out_matches (optional) = number of mask hits. */
int pst_buffer_filter_into(const pst_buffer* src, pst_buffer* dst, const uint8_t* mask, uint32_t mask_memkind, int64_t num_matches_hint,
                           size_t* out_matches);
/* stream-ordered variant for callers that know the count (`Some(num_matches)`, as the reference's bench passes it,
 * benches/buffer_filter_bench.rs:62-74): count, scan and copies are enqueued on the current stream and the call returns; no host
 * synchronisation, no panic mapping.  The mask is a device pointer.  At most num_matches points are written; the number of mask hits
 * is copied to *device_count_out (device-accessible memory, optional) in stream order -- a value above num_matches is the
 * reference's slice panic (:1103-1108) and the caller's to check.  dst->len < num_matches -> PST_ERR_RANGE (checked on the host). */
int pst_buffer_filter_into_async(const pst_buffer* src, pst_buffer* dst, const uint8_t* device_mask, size_t num_matches, uint64_t* device_count_out);
/* HashMapBuffer::filter::<B, _> (point_buffer.rs:1064-1076): new buffer of out_storage holding exactly the matching points */
int pst_buffer_filter(const pst_buffer* src, const uint8_t* mask, uint32_t mask_memkind, uint32_t out_storage, pst_buffer** out);

/* ---- device expressions: user-written closures as source text (round 5) -----------------------------------------------------------------
 * The reference takes ANY closure: Fn(T) -> T transformations (buffer_conversion.rs:13-36, 194-234), transform_attribute's Fn(usize, T) -> T
 * (point_buffer.rs:391-404) and filter's Fn(usize) -> bool (point_buffer.rs:1064-1136).  A closure cannot cross a C ABI into a kernel; its
 * source text can.  An expression is C++ EXPRESSION syntax (no statements, no braces, no string literals) over these names, compiled at run
 * time with hipRTC (cached per text; -ffp-contract=off: `v * s + o` keeps its two roundings) and run as a device function:
 *   transformations:  v = this component of the value (of T's component type; the value itself for scalars),  x y z = the components of a
 *                     Vec3 value,  c = the component being computed (0 1 2),  i = the point's index (the closure's usize),  p0 .. p3 = device
 *                     arrays of double given with the call (what a closure would capture).  One expression serves every component; a Vec3
 *                     attribute may give three, `x-expr ; y-expr ; z-expr`.  The result is converted to T's component type with Rust `as`.
 *   predicates:       every attribute of the buffer's layout whose name is a C identifier -- scalars by value, Vec3 as .x .y .z --, i, p0 .. p3:
 *                     "Classification == 2 && Position3D.z < 120.0".
 * Results are those of the same arithmetic on the host, bit for bit, EXCEPT which NaN an operation returns: sign and payload of a NaN result
 * are unspecified in Rust and differ between gfx950 and x86 (`y - z` with a NaN z: the GPU evaluates y + (-z) and returns the NaN with its sign
 * flipped); a NaN is a NaN on both.
 * Scalar and Vec3 attributes only.  A text that does not compile is PST_ERR_UNSUPPORTED_TRANSFORM with the compiler's log in pst_last_error;
 * PST_JIT=0 (no run-time compiler) makes every expression PST_ERR_UNSUPPORTED_TRANSFORM.  The closed descriptors (pst_transform) remain the
 * fast path for the in-tree callers' closures; an expression mapping is its own strided launch. */
/* BufferLayoutConverter::set_custom_mapping_with_transformation (buffer_conversion.rs:194-234) with the closure as an expression; T = the
 * source attribute's datatype when apply_to_source (the conversion follows), the target's otherwise (the conversion precedes) :209-213 */
int pst_converter_set_custom_mapping_with_expression(pst_converter* c, const char* from_name, const pst_datatype* from_dt, const char* to_name,
                                                     const pst_datatype* to_dt, const char* expr, int apply_to_source);
/* BorrowedMutBufferExt::transform_attribute(attribute, |index, value| expr), point_buffer.rs:391-404, in place; device_params = up to four
 * device arrays of double the expression names p0 .. p3 (NULL / 0 for none) */
int pst_transform_attribute_expr(pst_buffer* b, const char* name, const pst_datatype* dt, const char* expr, const double* const* device_params, size_t n_params);
/* HashMapBuffer::filter(|index| expr) -> new buffer of out_storage holding exactly the matching points (point_buffer.rs:1064-1076) */
int pst_buffer_filter_expr(const pst_buffer* src, const char* expr, const double* const* device_params, size_t n_params, uint32_t out_storage, pst_buffer** out);
/* the translation unit an expression becomes (kind 0: transformation between src_dt / dst_dt; kind 1: predicate over `layout`): what a compile
 * error's line numbers refer to, and what the CPU tests hand to pst_jit_compile_source.  *needed = its size, terminator included. */
int pst_expr_source(int kind, const pst_layout* layout, const pst_datatype* src_dt, const pst_datatype* dst_dt, int apply_to_source, const char* expr, char* buf,
                    size_t cap, size_t* needed);

/* RawPointConverter::{from_to, convert}, pasture-core/src/layout/conversion/attribute_conversion.rs:62-109 — the point-major variant:
 * one `as` converter per attribute present in BOTH layouts (matched by name, in the order of `from`) whose datatypes differ.
 * Attributes with equal datatypes get no converter and are SKIPPED, not copied (:73-90); an impossible pair is the panic of :267-269
 * (PST_ERR_INVALID_CONVERSION).  `convert` runs the converters on `count` interleaved points (the reference converts one point slice
 * per call); bytes of the target points that no converter writes keep their values.  Both buffers must be interleaved and carry the
 * layouts given to create (the reference's `unsafe` contract, checked here: PST_ERR_LAYOUT_MISMATCH). */
int pst_point_converter_create(const pst_layout* from, const pst_layout* to, pst_point_converter** out);
int pst_point_converter_destroy(pst_point_converter* c);
int pst_point_converter_num_converters(const pst_point_converter* c, size_t* out);
int pst_point_converter_convert(const pst_point_converter* c, const pst_buffer* src, size_t src_first, pst_buffer* dst, size_t dst_first, size_t count);
/* ---- BufferLayoutConverter ------------------------------------------------------------------------- */
int pst_converter_create(const pst_layout* from, const pst_layout* to, int with_default, pst_converter** out); /* for_layouts :112 / for_layouts_with_default :126 */
int pst_converter_destroy(pst_converter* c);
int pst_converter_set_custom_mapping(pst_converter* c, const char* from_name, const pst_datatype* from_dt, const char* to_name,
                                     const pst_datatype* to_dt);                                       /* :156-183 */
int pst_converter_set_custom_mapping_with_transformation(pst_converter* c, const char* from_name, const pst_datatype* from_dt,
                                                         const char* to_name, const pst_datatype* to_dt, const pst_transform* xf,
                                                         int apply_to_source);                         /* :194-234 */
int pst_converter_num_mappings(const pst_converter* c, size_t* out);
int pst_converter_get_mapping(const pst_converter* c, size_t index, pst_mapping_info* out);
/* convert_into_range :292-359 (convert_into :268 = full ranges). Enqueues on the current stream, then synchronises. */
int pst_converter_convert_into_range(const pst_converter* c, pst_buffer* src, size_t s0, size_t s1, pst_buffer* dst, size_t t0, size_t t1);
int pst_converter_convert_into_range_async(const pst_converter* c, pst_buffer* src, size_t s0, size_t s1, pst_buffer* dst, size_t t0, size_t t1);
/* convert :242-259 — allocates the target (new_from_layout + resize) and converts into it */
int pst_converter_convert(const pst_converter* c, pst_buffer* src, uint32_t out_storage, pst_buffer** out);
/* convert_into_range followed by calculate_bounds(target range) in ONE pass over HBM when the mapping set allows
 * (columnar Vec3f64 POSITION_3D target); identical results to the two separate calls. */
int pst_converter_convert_into_range_with_bounds(const pst_converter* c, pst_buffer* src, size_t s0, size_t s1, pst_buffer* dst,
                                                 size_t t0, size_t t1, double out_min[3], double out_max[3], int* has_value);
/* stream-ordered variant: the result record {min[3], max[3]} (6 doubles; seeds +/-f64::MAX if the range is empty)
 * is written to `device_out6` (device-accessible memory); no host synchronisation, no panic mapping. */
int pst_converter_convert_into_range_with_bounds_async(const pst_converter* c, pst_buffer* src, size_t s0, size_t s1, pst_buffer* dst,
                                                       size_t t0, size_t t1, double* device_out6);

/* ---- plan specialisation ------------------------------------------------------------------------------
 * The reference's converter is layout-generic (buffer_conversion.rs:112-234) and walks its Vec<AttributeMapping> at run time.  Here a
 * conversion takes one of these kernel families; pst_last_plan_kinds reports (one bit per family, 1u << PST_PLAN_*) which ones the calling
 * thread's last pst_converter_convert* call launched.  PST_PLAN_JIT: the mapping list compiled into the kernel as a constant -- hipRTC at run
 * time, cached per plan in memory and on disk (PST_JIT = 0 | async (default: compiled on a background thread once a call of at least
 * PST_JIT_MIN_POINTS points has shown the plan, interpreted until then) | sync; PST_JIT_CACHE_DIR).  Results are identical whichever
 * family runs. */
enum {
  PST_PLAN_NONE = 0,
  PST_PLAN_INTERPRETED = 1, /* generic LDS-tile kernels interpreting the mapping list */
  PST_PLAN_JIT = 2,         /* the plan as a compile-time constant, compiled at run time */
  PST_PLAN_STATIC = 3,      /* the same kernels instantiated in-tree for the layouts of the reference's own benches */
  PST_PLAN_LAS = 4,         /* LAS-format-specialised decoder / transposer (raw_readers.rs:31-167, las_types.rs) */
  PST_PLAN_STREAM = 5,      /* columnar Vec3f64 stream kernel (copy / affine / AABB) */
  PST_PLAN_COLUMN = 6,      /* one wide-vector launch per columnar -> columnar mapping */
  PST_PLAN_COPY = 7,        /* identity between equal packed layouts: one byte copy of the records */
  PST_PLAN_DIRECT = 8,      /* strided fall-back without LDS staging (records too large for a tile) */
  PST_PLAN_EXPRESSION = 9   /* an expression mapping's OWN strided pass (one launch per mapping: columns -> columns, ragged tails, plans without a
                               specialised form); an expression that runs INSIDE the plan-specialised kernel reports PST_PLAN_JIT only */
};
int pst_last_plan_kinds(uint32_t* mask);
/* Compiles (or fetches from the cache) the specialised kernel for conversions between buffers of these storage kinds NOW, so that the first
 * call already takes it.  *plan_kind: the family such a call will use (PST_PLAN_JIT when a specialised kernel is ready). */
int pst_converter_prepare(const pst_converter* c, int src_columnar, int dst_columnar, int with_bounds, uint32_t* plan_kind);
/* Two families can serve LAS-shaped plans (typed LasPointFormatN records -> columns and columns -> records; raw LAS records -> typed records): the
 * format-specialised LAS kernels and the plan-specialised kernel.  Which one is faster differs from box to box by a few per cent, so the
 * converter MEASURES it once per storage pairing on the first SYNCHRONOUS conversion of at least 2^22 points (convert / convert_into_range /
 * ..._with_bounds; both families run on the caller's range -- they write the same bytes --, median of three timed passes each, one host wait; not
 * while the stream is being captured, not when source and target memory overlap; PST_FAMILY_AUTOTUNE=0: never, plan-specialised first) and
 * keeps the winner.  The stream-ordered `_async` entry points never measure (they neither block the host nor repeat the caller's conversion):
 * callers of those run pst_converter_measure_families once, before their loop.
 * dst_columnar: 0 = records from records, 1 = columns (from records), 2 = records from columns.  *choice: -1 not measured yet, 0 = PST_PLAN_LAS,
 * 1 = plan-specialised (PST_PLAN_STATIC / PST_PLAN_JIT), 2 = the plan has no second family; ms2 (optional): milliseconds per pass the
 * measurement saw for {LAS, plan-specialised}.  (No reference counterpart: the reference has one loop, buffer_conversion.rs:292-359.) */
int pst_converter_family_choice(const pst_converter* c, int dst_columnar, int with_bounds, int* choice, float ms2[2]);
int pst_converter_measure_families(const pst_converter* c, pst_buffer* src, size_t s0, size_t s1, pst_buffer* dst, size_t t0, size_t t1, int with_bounds);
/* Introspection of the run-time compiler (tests, tools): the translation unit generated for a converter (empty when the plan takes another
 * family; *needed = bytes incl. the terminator); compilation of a translation unit against the embedded device headers for gfx950 WITHOUT a
 * device (the code object is copied to code_buf when given; *code_bytes = its size); counters. */
int pst_converter_jit_source(const pst_converter* c, int src_columnar, int dst_columnar, int with_bounds, char* buf, size_t cap, size_t* needed);
int pst_jit_compile_source(const char* source, void* code_buf, size_t code_cap, size_t* code_bytes, char* log, size_t log_cap);
typedef struct pst_jit_stats {
  uint64_t compiled, disk_hits, memory_hits, failures, launches;
  double compile_seconds;
} pst_jit_stats;
int pst_jit_get_stats(pst_jit_stats* out);
int pst_jit_set_mode(int mode); /* -1: back to the PST_JIT environment setting; 0 off; 1 async; 2 sync (tests, A/B harnesses) */

/* ---- pasture-algorithms loops --------------------------------------------------------------------- */
/* calculate_bounds, pasture-algorithms/src/bounds.rs:11-85.  has_value = 0 <=> None. */
int pst_calculate_bounds(const pst_buffer* b, double out_min[3], double out_max[3], int* has_value);
int pst_calculate_bounds_async(const pst_buffer* b, double* device_out6);
/* minmax_attribute::<T>, pasture-algorithms/src/minmax.rs:13-51 with T = `dt` (must be the stored datatype) */
int pst_minmax_attribute(const pst_buffer* b, const char* name, const pst_datatype* dt, void* out_min, void* out_max, int* has_value);
/* BorrowedMutBufferExt::transform_attribute, point_buffer.rs:391-404, with a closed-set transformation */
int pst_transform_attribute(pst_buffer* b, const char* name, const pst_datatype* dt, const pst_transform* xf);
/* compute_centroid, pasture-algorithms/src/normal_estimation.rs:198-237: mean of Position3D (Vec3f64) over all points, or over the
 * finite ones when some coordinate is NaN (is_dense :133-140).  Empty buffer -> PST_ERR_TOO_FEW_POINTS ("The point cloud is empty!").
 * A parallel sum: equal to the reference's left-to-right sum within rounding (1e-9 relative), not bit for bit. */
int pst_compute_centroid(const pst_buffer* b, double out_centroid[3]);
/* compute_normals, pasture-algorithms/src/normal_estimation.rs:79-130: per point (normal[3] f64, curvature f64) to
 * host arrays; out_knn (nullable, n*k int64, -1 padded) receives the neighbour indices in ascending distance. */
int pst_compute_normals(const pst_buffer* b, size_t k, double* out_normals, double* out_curvature, int64_t* out_knn);
/* device-resident variant: writes the NORMAL attribute (Vec3f32, point_layout.rs:594-597; f64 -> f32 `as` narrowing)
 * and an F64 "Curvature" attribute of `dst` (columnar or interleaved, same length) without leaving HBM. */
int pst_compute_normals_into(const pst_buffer* b, size_t k, pst_buffer* dst);
/* the same result as pst_compute_normals in caller-owned DEVICE memory (each pointer nullable, at least one given): normals f64 [n][3],
 * curvature f64 [n], neighbour lists uint32 [n][k] in ascending distance (normal_estimation.rs:103-108; 0xFFFFFFFF pads clouds of
 * fewer than k points).  10^8 points, k = 16: 2.4 GB + 0.8 GB + 6.4 GB. */
int pst_compute_normals_device(const pst_buffer* b, size_t k, double* d_normals, double* d_curvature, uint32_t* d_knn);
/* Stream-ordered compute_normals (round 4).  The synchronous call measures the cloud between its kernels (bounds, occupancy, local scale, a
 * probe and a census of the built index) and reads five to eight values back; pst_compute_normals_plan_create runs it ONCE (dst holds the
 * result) and keeps what it decided -- the grid's frame, box and cell edges, the LDS box shape, the capacities of the occupied-box list and
 * of the hand-back list.  pst_compute_normals_into_async then runs keys -> sort -> permutation -> directory -> box search -> exact search of
 * the hand-backs on the current stream with no host round trip and no allocation (hipGraph-capturable), on this cloud or on ANOTHER cloud of
 * the same length: the grid is fixed by the plan, points outside it are clamped into boundary cells and their queries go to the exact
 * search, so the result is exact for any data.  device_status2[0] = 0 when it is complete; bit 0: the number of finite points differs from
 * the plan's, bit 1 / bit 2: more occupied boxes / more hand-backs than the plan provided for, bit 3: the exact search handed queries back
 * (far points: the coarser levels are host-driven), bit 4: degenerate neighbourhoods ([1] = how many: PST_ERR_NOT_ENOUGH_NEIGHBOURS of the
 * synchronous call) -- with any of bits 0-3 set the caller falls back to pst_compute_normals_into.  Clouds whose synchronous call did not
 * take the box search or left queries open have no plan: PST_ERR_UNSUPPORTED with the reason in the message.  The box search is taken
 * by clouds that fill their bounding box (from a few thousand points on: 10^5 points have a plan for every k from 3 to 64) and by
 * larger clouds that do not but fit its directory budget; brute-force clouds, clouds with non-finite points or far outliers have none. */
typedef struct pst_normals_plan pst_normals_plan;
int pst_compute_normals_plan_create(const pst_buffer* b, size_t k, pst_buffer* dst, pst_normals_plan** out);
int pst_normals_plan_destroy(pst_normals_plan* plan);
int pst_compute_normals_into_async(pst_normals_plan* plan, const pst_buffer* b, pst_buffer* dst, uint64_t* device_status2);
/* voxelgrid_filter, pasture-algorithms/src/voxel_grid.rs:109-166: one centroid point per occupied voxel (cells centred on the
 * axis markers min + k*leafsize, find_leaf :21-52), appended to `filtered` in (x, y, z) voxel order.  Reductions per attribute
 * of filtered's layout (set_all_attributes :459-689): average (Position3D, ColorRGB, Normal, Intensity, NIR; sequential f64
 * sums in point order), most common (return fields, classification, scan angle, user data, point source id; ties: smallest
 * value — the reference's HashMap order is random), max-pool from 0.0 (ClassificationFlags, GpsTime, PointID).
 * Panics: no Position3D -> PST_ERR_MISSING_ATTRIBUTE; empty buffer -> PST_ERR_BOUNDS_INVALID (unwrap on None); waveform or
 * non-standard attribute in filtered's layout -> PST_ERR_UNSUPPORTED_ATTRIBUTE; attribute missing in `buffer` -> PST_ERR_MISSING_ATTRIBUTE.
 * filtered's length is final on return; the attribute reductions are enqueued on the current stream (no final synchronisation). */
int pst_voxelgrid_filter(const pst_buffer* buffer, double leafsize_x, double leafsize_y, double leafsize_z, pst_buffer* filtered);

/* Stream-ordered voxelgrid_filter (round 4).  pst_voxelgrid_filter reads three things back between its kernels (the bounds for the axis
 * markers, the voxel count for the output, the count of very large voxels): on a busy host each round trip costs more than the kernels.
 * pst_voxelgrid_plan_create runs ONE synchronous pass over `buffer` and allocates every scratch buffer for capacities derived from it (points
 * = len(buffer); an eighth more axis markers, a quarter more occupied voxels: *max_voxels).  pst_voxelgrid_filter_async then enqueues
 * calculate_bounds -> markers (create_markers_for_axis :55-83 by one lane: the same sequential additions) -> keys -> sort -> run heads ->
 * reductions on the current stream with NO host synchronisation and NO allocation (hipGraph-capturable); one centroid per occupied voxel
 * lands in filtered[dst_first ..) (filtered must already hold dst_first + max_voxels points; the tail behind the count is not written),
 * device_count_and_status[0] = number of voxels, [1] = status: 0 = the result is the reference's; bit 0 bounds invalid (an all-NaN
 * component: the reference panics), bit 1 more axis markers than planned, bit 2 more voxels than planned, bit 3 a leaf size that does not
 * advance the markers -- with any bit set nothing useful was written and the caller falls back to pst_voxelgrid_filter.  The buffer may be
 * ANOTHER cloud of the same length (the plan fixes capacities, not contents).  One call per plan in flight at a time. */
typedef struct pst_voxel_plan pst_voxel_plan;
int pst_voxelgrid_plan_create(const pst_buffer* buffer, double leafsize_x, double leafsize_y, double leafsize_z, pst_voxel_plan** out, size_t* max_voxels);
int pst_voxelgrid_plan_destroy(pst_voxel_plan* plan);
int pst_voxelgrid_filter_async(pst_voxel_plan* plan, const pst_buffer* buffer, pst_buffer* filtered, size_t dst_first, uint64_t* device_count_and_status);

/* ---- RANSAC plane / line segmentation (pasture-algorithms/src/segmentation.rs:117-370) ------------------------------------------
 * ransac_plane_serial / ransac_line_serial with the two halves of the reference's loop separated at the random numbers, which come from
 * rand::thread_rng() there and cannot be reproduced: *_fit scores hypotheses built from point indices the CALLER names, the sampler
 * produces such indices from a seed, and the seeded entry points are the sampler followed by *_fit, nothing more.
 * Position3D must be stored as Vec3f64 (view_attribute::<Vector3<f64>>: anything else -> PST_ERR_MISSING_ATTRIBUTE); interleaved or columnar,
 * owned, sliced or external.  Models cross the boundary as plain arrays: double plane[4] = a, b, c, d of ax + by + cz + d = 0 (not
 * normalised); double line[6] = first xyz, second xyz.
 *   plane from (i1, i2, i3):  v1 = p2 - p1, v2 = p3 - p1, n = v1 x v2, d = -(n . p1)                                   (:60-75)
 *   plane inlier:  |a*x + b*y + c*z + d| / sqrt(a*a + b*b + c*c) < distance_threshold                                    (:31-35)
 *   line inlier:   |(second - first) x (first - p)| / |second - first| < distance_threshold                              (:39-44)
 * every operation a separately rounded f64 operation, left to right, the division included; cross = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x), dot = (a.x*b.x + a.y*b.y) + a.z*b.z, norm = sqrt((x*x + y*y) + z*z) (asserted of nalgebra, unverified).
 * Degenerate hypotheses (collinear or coincident samples) and NaN coordinates fall out of IEEE arithmetic: no inliers.  The ranking of a
 * hypothesis is its number of inliers; the result is the hypothesis with the highest ranking, the LAST such iteration on ties
 * (Iterator::max_by of ransac_*_serial; rayon's choice in *_par is unspecified).
 * Status codes: fewer than 3 (plane) / 2 (line) points -> PST_ERR_TOO_FEW_POINTS (the reference's panics :119-121, :98); iterations == 0 ->
 * PST_ERR_INVALID_ARGUMENT (unwrap of an empty max_by); a sample index >= len -> PST_ERR_RANGE; equal indices inside one hypothesis ->
 * PST_ERR_INVALID_ARGUMENT (the reference's redraw loops make them impossible); 2^32 - 1 points and more, or 2^32 iterations and more ->
 * PST_ERR_UNSUPPORTED.  Null arguments and iterations == 0 are answered before a device is looked for. */
/* Host only, no device needed.  Fills out_indices[iterations * per_hypothesis] (per_hypothesis = 3 plane, 2 line).  The recipe: ONE counter c
 * per call starts at 0 and advances by one with every draw; draw() = (splitmix64(seed ^ c) * n_points) >> 64 (the 128-bit product; splitmix64 =
 * the finaliser of pst_buffer_synth_fill: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) *
 * 0x94D049BB133111EB; x ^ x >> 31).  Per iteration: r1 = draw(); r2 = draw(), redrawn while r2 == r1; for a plane r3 = draw(), redrawn while
 * r3 == r2 or r3 == r1 (:50-58, :82-87).  n_points < per_hypothesis -> PST_ERR_TOO_FEW_POINTS (the loops would not end). */
int pst_ransac_sample_indices(uint64_t seed, size_t n_points, size_t iterations, uint32_t per_hypothesis, uint64_t* out_indices);
/* samples: host, iterations * 3 (plane) / * 2 (line) point indices.  Returns the winning model, its ranking, (optional) which iteration won and
 * (optional) rankings[iterations] of every hypothesis.  The positions are read once per batch of hypotheses, not once per hypothesis. */
int pst_ransac_plane_fit(const pst_buffer* b, double distance_threshold, const uint64_t* samples, size_t iterations, double plane[4], uint64_t* ranking,
                         size_t* best_iteration, uint64_t* rankings);
int pst_ransac_line_fit(const pst_buffer* b, double distance_threshold, const uint64_t* samples, size_t iterations, double line[6], uint64_t* ranking,
                        size_t* best_iteration, uint64_t* rankings);
/* pst_ransac_sample_indices(seed, len, iterations, 3 | 2) followed by *_fit */
int pst_ransac_plane(const pst_buffer* b, double distance_threshold, size_t iterations, uint64_t seed, double plane[4], uint64_t* ranking);
int pst_ransac_line(const pst_buffer* b, double distance_threshold, size_t iterations, uint64_t seed, double line[6], uint64_t* ranking);
/* The inliers of a model (the Vec<usize> of the reference's result), ascending.  *count = their number -- equal to the ranking *_fit returned
 * for the same model and threshold (one device function serves every kernel).  indices (host, optional) receives them when they fit
 * `capacity`; more inliers than that -> PST_ERR_RANGE with *count still set.  An empty buffer has none (answered on the host). */
int pst_plane_inliers(const pst_buffer* b, const double plane[4], double distance_threshold, uint64_t* indices, size_t capacity, uint64_t* count);
int pst_line_inliers(const pst_buffer* b, const double line[6], double distance_threshold, uint64_t* indices, size_t capacity, uint64_t* count);
/* The same predicate as a byte mask (1 = inlier) of len bytes in DEVICE memory, stream-ordered, no host synchronisation: what
 * pst_buffer_filter_into(..., PST_MEM_DEVICE, ranking, ...) and pst_buffer_filter_into_async take. */
int pst_plane_inlier_mask_device(const pst_buffer* b, const double plane[4], double distance_threshold, uint8_t* device_mask);
int pst_line_inlier_mask_device(const pst_buffer* b, const double line[6], double distance_threshold, uint8_t* device_mask);
/* The scoring kernel's seams (tests place their sizes around them; each pointer optional): points one wave holds in registers, points per
 * workgroup, workgroups per compute unit of one grid pass, hypotheses scored per pass over the positions.  Host only. */
int pst_ransac_kernel_shape(uint32_t* points_per_wave, uint32_t* points_per_block, uint32_t* blocks_per_cu, uint32_t* batch);

/* ---- kNN search and outlier removal -------------------------------------------------------------------------------------------------
 * The neighbour search of compute_normals as an entry point of its own, with the neighbour DISTANCES, and the two outlier criteria every
 * LiDAR pipeline runs between "read" and "normals" (the definitions of PCL's / PDAL's StatisticalOutlierRemoval and RadiusOutlierRemoval;
 * the reference has neither).  The masks are one byte per point, 1 = keep: what pst_buffer_filter / pst_buffer_filter_into take.
 * Checks and limits of pst_compute_normals_device: fewer than 3 points -> PST_ERR_TOO_FEW_POINTS, k < 3 -> PST_ERR_K_TOO_SMALL, Position3D
 * not stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE, k > 64 or 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED; interleaved or columnar,
 * owned, sliced or external.  Degenerate plane fits are NOT an error here (no plane is asked for).  Null arguments and invalid parameters are
 * answered before a device is looked for, the cloud's length after it; without a device every call is PST_ERR_NO_DEVICE, never a CPU path.
 * All three calls are synchronous (the search is host-driven).
 *   distance of slot t of query q, neighbour p:  dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;  d = sqrt((dx*dx + dy*dy) + dz*dz),
 * every operation a separately rounded f64 operation.  A padded slot (index 0xFFFFFFFF: clouds of fewer than k points) has distance +inf;
 * non-finite coordinates give what IEEE arithmetic gives. */
/* d_knn (device, nullable): uint32 [n][k], exactly what pst_compute_normals_device writes.  d_dist (device, required): f64 [n][k]. */
int pst_knn_search_device(const pst_buffer* b, size_t k, uint32_t* d_knn, double* d_dist);
/* Statistical outlier removal.  Per point dbar = (d[1] + d[2] + ... + d[mean_k]) / (double)mean_k over its list in ascending distance, summed
 * left to right; slot 0 (the query or a coincident point, distance 0 either way) is skipped, so dbar depends on the sorted multiset of
 * distances only.  The search runs with k = max(mean_k + 1, 3).  Over the m points whose dbar is finite: mean = sum(dbar) / m,
 * stddev = sqrt(sum((dbar - mean)^2) / (m - 1)) in a second pass (0 when m < 2), threshold = mean + stddev_mult * stddev;
 * stats = {mean, stddev, threshold, (double)m}.  mask[i] = 1 iff dbar_i is finite and dbar_i <= threshold; *kept = their number.  Both sums
 * are fixed-shape reductions (blocks of a fixed number of points, a fixed tree per block, the block partials added in block order by one
 * workgroup, no floating-point atomics): two calls on one cloud give the same bits.  mask: len bytes in device memory (mask_memkind =
 * PST_MEM_DEVICE) or host memory (anything else), the convention of pst_buffer_filter_into.  d_mean_dist (device, nullable): f64 [n], dbar.
 * mean_k outside 1 .. 63 or a NaN stddev_mult -> PST_ERR_INVALID_ARGUMENT; fewer than mean_k + 1 points -> PST_ERR_TOO_FEW_POINTS. */
int pst_statistical_outlier_mask(const pst_buffer* b, size_t mean_k, double stddev_mult, uint8_t* mask, uint32_t mask_memkind, double* d_mean_dist, double stats[4],
                                 uint64_t* kept);
/* Radius outlier removal.  mask[i] = 1 iff at least min_neighbours points other than point i itself lie within `radius` of it, that is iff
 * d[i][min_neighbours] <= radius; a padded slot or a NaN distance compares false, so a cloud of min_neighbours points or fewer keeps nothing.
 * The search runs with k = max(min_neighbours + 1, 3).  min_neighbours outside 1 .. 63, a negative or non-finite radius ->
 * PST_ERR_INVALID_ARGUMENT. */
int pst_radius_outlier_mask(const pst_buffer* b, double radius, size_t min_neighbours, uint8_t* mask, uint32_t mask_memkind, uint64_t* kept);
/* The kernels' seams (tests place their sizes around them; each pointer optional): points whose whole neighbour lists one workgroup of the
 * distance kernels owns (whatever k), threads of the one workgroup that adds the block partials of the sums (each a contiguous run of them),
 * points per block partial.  Host only. */
int pst_outlier_kernel_shape(uint32_t* points_per_block, uint32_t* reduce_block, uint32_t* reduce_points_per_block);

/* ---- Euclidean cluster extraction (radius connected components) ----------------------------------------------------------------------
 * What PCL's EuclideanClusterExtraction / PDAL's filters.cluster compute (the reference has neither): the points are split into connected
 * groups, "two points belong together when they are closer than a tolerance", and the groups come back largest first.  The definition:
 *   finite point:  all three coordinates of its Position3D (Vec3f64) are finite; a point with a NaN or +-inf coordinate is in no cluster.
 *   adjacency:     finite points i and j are adjacent iff (dx*dx + dy*dy) + dz*dz <= t2, dx = pj.x - pi.x (y, z alike), every operation a
 *                  separately rounded f64 operation, t2 = tolerance * tolerance rounded once on the host.  There is no sqrt: this differs
 *                  from sqrt(d2) <= tolerance only where d2 and t2 lie within an ulp or two of each other (sqrt rounds once more, and a d2
 *                  just above t2 can round down onto the tolerance).
 *   cluster:       a connected component of that graph -- it depends on nothing else: not on the grid, the traversal order or the schedule.
 *   size filter:   clusters of fewer than min_size or more than max_size points are dropped; their points are in no cluster.
 *   numbering:     the kept clusters are numbered 0, 1, ... by descending size, ties by ascending smallest member index (index in the
 *                  buffer): cluster 0 is the largest.
 *   labels:        labels[i] = the cluster number of point i, or 0xFFFFFFFF when it is in none.
 * Two calls on one cloud write the same bytes (sizes are integer sums, the numbering is a stable sort).
 * Position3D not stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE; interleaved or columnar, owned, sliced or external, at any byte offset.
 * tolerance not finite, not > 0 or with tolerance * tolerance not a normal number, min_size == 0, min_size > max_size ->
 * PST_ERR_INVALID_ARGUMENT; 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED (so is a cloud whose finite extent overflows f64).  Null
 * arguments and invalid parameters are answered before a device is looked for, the cloud's length after it; without a device the call is
 * PST_ERR_NO_DEVICE, never a CPU path.  Any length from 0 up is legal: an empty cloud has no clusters (answered on the host).
 * Cost: every point tests the points of its own and the neighbouring grid cells (cell edge just above the tolerance), about 27 x the mean
 * cell occupancy / 2 pair tests per point -- a tolerance far above the point spacing is quadratic per cell. */
/* Synchronous.  labels: len x uint32 in device memory (labels_memkind = PST_MEM_DEVICE) or host memory (anything else), the convention of
 * the outlier masks.  sizes (host, nullable): sizes[c] = points of kept cluster c, when the kept clusters fit sizes_capacity; more kept
 * clusters than that -> PST_ERR_RANGE with *n_clusters and *n_clustered set and the labels written (the pst_plane_inliers convention).
 * *n_clusters = kept clusters, *n_clustered = points that carry a label (the sum of the kept sizes). */
int pst_euclidean_clusters(const pst_buffer* b, double tolerance, uint64_t min_size, uint64_t max_size, uint32_t* labels, uint32_t labels_memkind,
                           uint64_t* sizes, size_t sizes_capacity, uint64_t* n_clusters, uint64_t* n_clustered);
/* d_mask[i] = 1 iff first_cluster <= d_labels[i] < first_cluster + cluster_count, else 0 (computed without wrapping: 0xFFFFFFFF, "no
 * cluster", is never selected).  Both arrays in DEVICE memory, n elements; stream-ordered, no host synchronisation: the mask is what
 * pst_buffer_filter_into(..., PST_MEM_DEVICE, ...) takes. */
int pst_cluster_mask_device(const uint32_t* d_labels, uint64_t n, uint32_t first_cluster, uint32_t cluster_count, uint8_t* d_mask);
/* The traversal kernel's seams (tests place their sizes around them; each pointer optional): points one workgroup owns (one lane each), points
 * of one LDS candidate tile -- 0: the kernel reads its candidates from the sorted position arrays directly and stages none.  Host only. */
int pst_cluster_kernel_shape(uint32_t* points_per_block, uint32_t* tile_points);
/* Measurement aid.  With PST_CLUSTER_TIMES=1 in the environment pst_euclidean_clusters brackets its three phases with stream events; this
 * returns the calling thread's last call: ms = {index build (AABB, keys, sort, gather), traversal + union, bookkeeping}.  Zeros without the
 * switch.  Host only. */
int pst_cluster_phase_times(double ms[3]);

/* ---- DBSCAN (core, border and noise points) ---------------------------------------------------------------------------------------------
 * What PDAL's filters.dbscan and scikit-learn's DBSCAN compute (the reference has neither): clusters are carried by the points that have
 * enough neighbours; points on the rim are attached to a cluster but never bridge two; the rest is noise.  Where pst_euclidean_clusters joins
 * everything that touches -- two objects linked by a thread of stray returns become one, every isolated return is a cluster of its own --
 * this call keeps the objects apart and the strays out.  The definition:
 *   finite point:  as for the clusters.  A point with a NaN or +-inf coordinate is neither core nor border, is nobody's neighbour, and gets
 *                  the label 0xFFFFFFFF.
 *   neighbour:     finite points i and j are neighbours iff (dx*dx + dy*dy) + dz*dz <= e2, dx = pj.x - pi.x (y, z alike), every operation a
 *                  separately rounded f64 operation, e2 = eps * eps rounded once on the host.  There is no sqrt.  This is the adjacency of
 *                  pst_euclidean_clusters and the conflict of pst_poisson_disk_mask, on purpose.  A finite point is its own neighbour.
 *   core:          finite point i is a core point iff the number of its neighbours, ITSELF INCLUDED, is >= min_points (scikit-learn's
 *                  min_samples, PDAL's min_points).
 *   cluster:       a connected component of the neighbour graph restricted to the CORE points.
 *   border:        a finite point that is not core and has at least one core neighbour.  It joins the cluster of the core neighbour with
 *                  the smallest d2 (the sum above), ties to the core neighbour with the smallest index in the buffer.  Nothing is united
 *                  through it.  Sequential DBSCAN gives a border point to whichever cluster reaches it first, which depends on the order
 *                  of the visit; this rule is the order-free choice.  Core points, noise points and the partition of the core points are
 *                  exactly scikit-learn's and PDAL's; only a border point within eps of two clusters may go to the other one there.
 *   noise:         every other point; label 0xFFFFFFFF.
 *   numbering:     the clusters are numbered 0, 1, ... by descending size (core + border members), ties by ascending smallest member index
 *                  (index in the buffer): the clusters' rule.  There is no size filter: min_points is the filter.
 * The result depends on nothing else: not on the grid, the schedule, the storage or the launch shape.  Two calls on one cloud write the same
 * bytes (sizes are integer sums, the border choice is a minimum, the numbering is a stable sort).  Two consequences:
 *   min_points == 1: labels and sizes are byte for byte those of pst_euclidean_clusters(eps, 1, UINT64_MAX) -- every finite point is core.
 *   min_points == 2: they are those of pst_euclidean_clusters(eps, 2, UINT64_MAX) -- every member of a component of two or more points has
 *                    at least two neighbours, so there are no border points, and the singletons are noise.
 * Null b, labels or counts, an invalid memkind, eps not finite, not > 0 or with eps * eps not a normal number, min_points == 0 ->
 * PST_ERR_INVALID_ARGUMENT, answered before a device is looked for; Position3D not stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE
 * (interleaved or columnar, owned, sliced or external, at any byte offset); without a device PST_ERR_NO_DEVICE, never a CPU path; 2^32 - 16
 * points and more -> PST_ERR_UNSUPPORTED (so is a cloud whose finite extent overflows f64).  Any length from 0 up is legal: an empty cloud
 * has zero counts (answered on the host); a cloud without a finite point gets all-0xFFFFFFFF labels, zero core bytes and zero counts;
 * min_points above the number of finite points is legal and makes everything noise.
 * Cost: the index build of pst_euclidean_clusters, one walk of the 27 neighbouring grid cells per point that stops at min_points neighbours,
 * the clusters' traversal over the core points, and one more walk of the 27 cells for every point that is not core. */
/* Synchronous.  labels: len x uint32, required; core: len bytes, nullable, 1 = core point, 0 otherwise (scikit-learn's
 * core_sample_indices_ as a mask that pst_buffer_filter takes).  Both in device memory (memkind = PST_MEM_DEVICE) or both in host memory
 * (anything else), the convention of the cluster labels.  sizes (host, nullable): sizes[c] = points of cluster c, when the clusters fit
 * sizes_capacity; more clusters than that -> PST_ERR_RANGE with the counts set and the labels written.
 * counts = {clusters, core points, labelled points (core + border)}.  pst_cluster_mask_device turns the labels into a filter mask. */
int pst_dbscan(const pst_buffer* b, double eps, uint64_t min_points, uint32_t* labels, uint8_t* core, uint32_t memkind, uint64_t* sizes,
               size_t sizes_capacity, uint64_t counts[3]);
/* The seam of the count, link and border kernels (tests place their sizes around it; the pointer is optional): points one workgroup owns,
 * one lane each.  Host only. */
int pst_dbscan_kernel_shape(uint32_t* points_per_block);
/* Measurement aid.  With PST_DBSCAN_TIMES=1 in the environment pst_dbscan brackets its four phases with stream events; this returns the
 * calling thread's last call: ms = {index build (AABB, keys, sort, gather), core count, link, border + bookkeeping}.  Zeros without the
 * switch.  Host only. */
int pst_dbscan_phase_times(double ms[4]);

/* ---- Region growing (smooth surface patches) ------------------------------------------------------------------------------------------------
 * What PCL's RegionGrowing, CloudCompare's facet extraction and PDAL pipelines built on filters.normal compute (the reference has none of
 * them): the cloud is split into its smooth surface patches -- roof faces, walls, the road, the sides of a box -- by joining neighbouring
 * points whose normals agree.  Where pst_euclidean_clusters and pst_dbscan group by distance alone, so that a building comes back as one
 * blob, this call separates what meets at an edge.  Every floating-point operation below is a separately rounded f64 operation;
 * tests/region_ref.py restates the definition in numpy.
 *   inputs:        n points; k in 1 .. 64; neighbour lists knn uint32 [n][k], which need not be sorted; normals f64 [n][3]; curvature
 *                  f64 [n], nullable; min_abs_cos in [0, 1]; curvature_threshold; max_distance (+inf: no limit); min_size >= 1 and
 *                  max_size >= min_size.
 *   valid point:   all three components of its normal are finite.  Any other point gets the label 0xFFFFFFFF and is nobody's neighbour.
 *   smooth point:  a valid point with curvature[i] <= curvature_threshold; a NaN curvature compares false.  Without a curvature array every
 *                  valid point is smooth.  Smooth points carry the regions, as core points carry the clusters of pst_dbscan.
 *   slot:          slot t of point i names j = knn[i][t] and COUNTS iff j < n (the 0xFFFFFFFF padding and any out-of-range index are
 *                  skipped and never dereferenced), j != i, j is valid, and max_distance == +inf or d <= max_distance with
 *                  d = sqrt((dx*dx + dy*dy) + dz*dz), dx = p_j.x - p_i.x (y, z alike): the slot distance of pst_knn_search_device.  A NaN d
 *                  compares false.  Positions are read only when max_distance is finite.
 *   agreement:     i and j agree iff fabs((ni.x*nj.x + ni.y*nj.y) + ni.z*nj.z) >= min_abs_cos.  The normals are taken as given: they are
 *                  neither normalised nor oriented, and the absolute value makes their orientation irrelevant, as in PCL.
 *   region:        a connected component of the undirected graph on the SMOOTH points in which {i, j} is an edge iff both are smooth, they
 *                  agree, and j is in a counting slot of i OR i is in a counting slot of j.  kNN lists are not symmetric; one direction is
 *                  enough for an edge.
 *   rim:           a valid point that is not smooth.  It joins the region of the first slot, in slot order, that counts, names a smooth
 *                  point and agrees with it; without such a slot it is in no region.  Nothing is united through a rim point.
 *   size filter:   the clusters' rule: sizes are smooth plus rim members; regions of fewer than min_size or more than max_size points are
 *                  dropped, their points are in no region.
 *   numbering:     the kept regions are numbered 0, 1, ... by descending size, ties by ascending smallest member index (index in the buffer).
 *   labels:        labels[i] = the region number of point i, or 0xFFFFFFFF when it is in none.
 * The result depends on nothing else: not on the schedule, the storage or the launch shape.  Two calls write the same bytes (sizes are integer
 * sums, the rim choice is the first slot in slot order, the numbering is a stable sort).
 * How this differs from PCL's RegionGrowing: PCL grows sequentially from the seed of lowest curvature; it reaches j only through lists that
 * contain j, and it gives a point to the first region that arrives at it, which depends on the order of the visit.  PCL may also start a
 * region from a point above the curvature threshold when no other seed is left.  This definition is the order-free closure of PCL's rule:
 * the edges between smooth points are the same (taken in either direction), so the partition of the smooth points is PCL's wherever PCL's
 * does not depend on its visiting order; only the rim points (PCL: whichever region reaches them first; here: the first agreeing slot) and
 * the seedless regions (PCL: may start from a point above the threshold; here: never) differ.  PCL's residual test is not part of it.
 * Null b, d_knn, d_normals, labels or counts, an invalid memkind, k outside 1 .. 64, min_abs_cos outside [0, 1] or NaN, a NaN
 * curvature_threshold, a NaN or negative max_distance, min_size == 0, max_size < min_size -> PST_ERR_INVALID_ARGUMENT; Position3D not stored
 * as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE (interleaved or columnar, owned, sliced or external, at any byte offset; the attribute is
 * required even when max_distance is +inf); all of these are answered before a device is looked for.  An empty buffer is PST_OK with zero
 * counts, answered on the host; without a device the call is PST_ERR_NO_DEVICE, never a CPU path; 2^32 - 16 points and more ->
 * PST_ERR_UNSUPPORTED.  A cloud without a valid normal gets all-0xFFFFFFFF labels, zero mask bytes and zero counts.
 * Cost: one coalesced pass over the n * k list elements with one 24-byte gather per slot whose both ends are smooth, the union-find over the
 * agreeing slots, one walk of its own list for every rim point, and the clusters' numbering. */
/* Synchronous: the host reads the number of regions before the numbering sort, as pst_dbscan does.  d_knn, d_normals, d_curvature: DEVICE
 * memory.  labels: len x uint32, required; smooth: len bytes, nullable, 1 = smooth point, 0 otherwise.  Both in device memory (memkind =
 * PST_MEM_DEVICE) or both in host memory (anything else), the convention of pst_dbscan.  sizes (host, nullable): sizes[c] = points of region
 * c, when the kept regions fit sizes_capacity; more kept regions than that -> PST_ERR_RANGE with the counts set and the labels written.
 * counts = {kept regions, smooth points, labelled points}.  pst_cluster_mask_device turns the labels into a filter mask. */
int pst_region_growing_from_knn(const pst_buffer* b, size_t k, const uint32_t* d_knn, const double* d_normals, const double* d_curvature,
                                double min_abs_cos, double curvature_threshold, double max_distance, uint64_t min_size, uint64_t max_size,
                                uint32_t* labels, uint8_t* smooth, uint32_t memkind, uint64_t* sizes, size_t sizes_capacity, uint64_t counts[3]);
/* The search of pst_geometric_features (the same lists, checks and limits: k = 3 .. 64, at least 3 points, fewer than 2^32 - 16, Vec3f64),
 * then its kernel for e3 (the normals) and PST_FEATURE_SURFACE_VARIATION = l3 / S (the curvature, PCL's) with the same max_distance, then
 * the steps of the call above on what they wrote.  A point with fewer than 3 valid neighbours has a NaN normal and is in no region.
 * d_normals f64 [n][3], d_curvature f64 [n], d_knn uint32 [n][k] (device, each nullable): also receive what the regions were grown from;
 * scratch otherwise.  The parameters are checked before a device is looked for, then the device, then the length: an empty buffer is PST_OK
 * with zero counts; one of 1 or 2 points is PST_ERR_TOO_FEW_POINTS. */
int pst_region_growing(const pst_buffer* b, size_t k, double min_abs_cos, double curvature_threshold, double max_distance, uint64_t min_size,
                       uint64_t max_size, uint32_t* labels, uint8_t* smooth, uint32_t memkind, uint64_t* sizes, size_t sizes_capacity,
                       uint64_t counts[3], double* d_normals, double* d_curvature, uint32_t* d_knn);
/* The link kernel's seams for this k (tests place their sizes around them; each pointer optional): points whose whole neighbour lists one
 * workgroup owns, and its threads (it walks the lists that many elements at a time).  k outside 1 .. 64 -> PST_ERR_INVALID_ARGUMENT.  Host
 * only. */
int pst_region_kernel_shape(size_t k, uint32_t* points_per_block, uint32_t* threads);
/* Measurement aid.  With PST_REGION_TIMES=1 in the environment both calls bracket their three phases with stream events; this returns the
 * calling thread's last call: ms = {search + features (zero from lists), classify + link, attach + numbering}.  Zeros without the switch.
 * Host only. */
int pst_region_phase_times(double ms[3]);

/* ---- Minimum-distance (Poisson-disk) subsampling ----------------------------------------------------------------------------------------
 * What PDAL's filters.sample, CloudCompare's "subsample by space" and lidR's decimate_points compute (the reference has none of them): a
 * subset of the ORIGINAL points in which no two are closer than a radius, as a byte mask that pst_buffer_filter / pst_buffer_filter_into
 * take -- unlike pst_voxelgrid_filter, which invents centroids and guarantees no spacing.  The definition:
 *   finite point:  as for the clusters.  A point with a NaN or +-inf coordinate is never kept and conflicts with nothing.
 *   conflict:      finite points i and j conflict iff (dx*dx + dy*dy) + dz*dz <= r2, dx = pj.x - pi.x (y, z alike), every operation a
 *                  separately rounded f64 operation, r2 = radius * radius rounded once on the host.  There is no sqrt.  This is the
 *                  adjacency of pst_euclidean_clusters, on purpose: a thinned cloud clustered at tolerance = radius is all singletons.
 *   priority key:  a uint64 per buffer index i.  PST_SAMPLE_SHUFFLED (0): splitmix64(seed ^ i), the finaliser written out at
 *                  pst_ransac_sample_indices -- a bijection on 64 bits, so keys never tie.  PST_SAMPLE_INDEX_ORDER (1): i itself, the seed
 *                  is ignored -- PDAL's filters.sample exactly: the first point is always kept.
 *   kept set:      finite i is kept iff no kept j with a smaller key conflicts with it -- the result of the sequential greedy pass in
 *                  ascending key order.  It is unique and depends on nothing else: not on the grid, the schedule, the storage or the number
 *                  of rounds.
 *   mask:          mask[i] = 1 kept, 0 otherwise.
 * Two calls on one cloud write the same bytes.
 * Null arguments, an invalid memory kind, an order above 1, a radius not finite, not > 0 or with radius * radius not a normal number ->
 * PST_ERR_INVALID_ARGUMENT, answered before a device is looked for; then Position3D not stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE
 * (interleaved or columnar, owned, sliced or external, at any byte offset); then the device: without one the call is PST_ERR_NO_DEVICE, never a
 * CPU path; then the length: 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED (so is a cloud whose finite extent overflows f64).  Any length
 * from 0 up is legal: an empty cloud keeps nothing (answered on the host, *kept = 0, *rounds = 0); a cloud without a finite point gets an
 * all-zero mask and 0 rounds.
 * Cost: the index build of pst_euclidean_clusters, then rounds.  In a round every still undecided point tests the points of its own and the
 * 26 neighbouring grid cells (cell edge just above the radius) -- a radius far above the point spacing is quadratic per cell, as for the
 * clusters -- and decides when every conflicting point of smaller key has decided.  Shuffled keys need about ten rounds whatever the input
 * order.  PST_SAMPLE_INDEX_ORDER is correct but SLOW on ordered input: along a scan line every point waits for its predecessor, so the
 * number of rounds grows with the length of the chains of conflicts (hundreds of rounds on scan-line ordered LiDAR). */
#define PST_SAMPLE_SHUFFLED 0u
#define PST_SAMPLE_INDEX_ORDER 1u
/* Synchronous.  mask: len bytes in device memory (mask_memkind = PST_MEM_DEVICE) or host memory (anything else), the convention of the
 * outlier masks.  *kept = the number of ones.  rounds (nullable): *rounds = launches of the decision kernel. */
int pst_poisson_disk_mask(const pst_buffer* b, double radius, uint32_t order, uint64_t seed, uint8_t* mask, uint32_t mask_memkind, uint64_t* kept,
                          uint32_t* rounds);
/* Host only, no device needed: keys[j] = the priority key of buffer index first + j, j < count (the keys of the definition above; first + j
 * wraps at 2^64).  count == 0 writes nothing; an order above 1 -> PST_ERR_INVALID_ARGUMENT. */
int pst_sample_priorities(uint32_t order, uint64_t seed, uint64_t first, uint64_t count, uint64_t* keys);
/* The decision kernel's seams (tests place their sizes around them; each pointer optional): active points one workgroup owns (one lane each),
 * times a lane looks at its point in one launch before it leaves it undecided.  Host only. */
int pst_sample_kernel_shape(uint32_t* points_per_block, uint32_t* sweeps_per_launch);
/* Measurement aid.  With PST_SAMPLE_TIMES=1 in the environment pst_poisson_disk_mask brackets its three phases with stream events; this
 * returns the calling thread's last call: ms = {index build (AABB, keys, sort, gather), decision rounds, mask write}.  Zeros without the
 * switch.  Host only. */
int pst_sample_phase_times(double ms[3]);

/* ---- Gather by index and sort orders (attribute, Morton, shuffle) ----------------------------------------------------------------------
 * What PDAL's filters.sort, filters.mortonorder, filters.randomize and filters.head / filters.tail do, and what the index lists of
 * pst_plane_inliers / pst_line_inliers (u64) and of the neighbour searches (u32) are for (the reference has none of it): points picked or
 * reordered on the device.  The definitions:
 *   gather:        dst[dst_first + j] = src[indices[j]] for j < count, every attribute, byte for byte.  The layouts are equal; either buffer
 *                  is interleaved or columnar, owned, sliced or external, at any byte offset.  Indices may repeat, count may be larger or
 *                  smaller than the length of src.  Interleaved to interleaved moves whole records, padding included; in the other three
 *                  pairings record padding of an interleaved dst keeps what it held.  Nothing outside the count target points is written.
 *   attribute key: of one scalar attribute, or of component 0 .. 2 of a Vec3 attribute.  Unsigned types: the value.  Signed types: the value
 *                  with the sign bit flipped.  f32 / f64: -0.0 is first taken as +0.0, then key = sign ? ~bits : bits | signbit; every NaN,
 *                  of either sign, has the all-ones key.  Ascending key order with ties in input order is numpy's
 *                  argsort(values, kind="stable").  Descending: key' = ~key for every key that is not a NaN key: NaNs stay last and ties
 *                  keep input order in both directions.
 *   Morton key:    dims = 2 (x, y: PDAL's filters.mortonorder) or 3; `bits` per axis, 1 .. 31 for 2-D, 1 .. 21 for 3-D, 0 = that maximum.
 *                  The AABB is taken over the points whose three coordinates are finite.  Per axis, on the host: inv = 2^bits / (max - min),
 *                  0 if max == min or the quotient is not finite.  Per point and axis: t = (p - min) * inv, two separately rounded f64
 *                  operations; c = t >= 2^bits ? 2^bits - 1 : t >= 0 ? floor(t) : 0.  Bit i of cx goes to key bit dims * i, of cy to
 *                  dims * i + 1, of cz to dims * i + 2.  A point with a coordinate that is not finite has the key 1 << 63: it sorts last.
 *   shuffle key:   splitmix64(seed ^ i), the key of PST_SAMPLE_SHUFFLED and of pst_sample_priorities.
 *   order:         the stable sort of the element numbers by key: order[j] = the index of the point that comes j-th.  A buffer in that order
 *                  is the gather by `order`.  Two calls write the same bytes.
 * Checks, in this order.  Null arguments, index_bits not 32 / 64, an invalid memory or storage kind, dims not 2 / 3, bits out of range, a
 * component beyond the datatype, a datatype that is not numeric (ByteArray, Custom, Vec4u8) -> PST_ERR_INVALID_ARGUMENT, answered before a
 * device is looked for; layouts that differ -> PST_ERR_LAYOUT_MISMATCH; the attribute absent (by name and datatype), or Position3D not stored
 * as Vec3f64 for the Morton order -> PST_ERR_MISSING_ATTRIBUTE; any byte range of src overlapping one of dst -> PST_ERR_INVALID_ARGUMENT
 * (there is no in-place permutation); dst_first + count > the length of dst -> PST_ERR_RANGE; count == 0 and empty buffers are then PST_OK
 * on the host; then the device: without one PST_ERR_NO_DEVICE, never a CPU path; then sort orders of 2^32 - 16 points and more ->
 * PST_ERR_UNSUPPORTED (a gather with 64-bit indices takes any length); last, the synchronous gathers only: an index >= the length of src ->
 * PST_ERR_RANGE with dst unchanged. */
/* Synchronous and validated.  indices: count u32 (index_bits 32) or u64 (64) values in device memory (indices_memkind = PST_MEM_DEVICE) or
 * host memory (anything else). */
int pst_buffer_gather(const pst_buffer* src, const void* indices, uint32_t index_bits, uint32_t indices_memkind, size_t count, pst_buffer* dst,
                      size_t dst_first);
/* Stream-ordered on the current stream: no host synchronisation, no allocation.  An index >= the length of src skips its target point;
 * device_skipped (device memory, nullable) receives the number of such entries. */
int pst_buffer_gather_async(const pst_buffer* src, const void* device_indices, uint32_t index_bits, size_t count, pst_buffer* dst, size_t dst_first,
                            uint64_t* device_skipped);
/* pst_buffer_gather into a new buffer of count points and out_storage (PST_STORAGE_*); *out is the caller's to destroy. */
int pst_buffer_take(const pst_buffer* src, const void* indices, uint32_t index_bits, uint32_t indices_memkind, size_t count, uint32_t out_storage,
                    pst_buffer** out);
/* The orders: d_order = len (n) u32 values in device memory.  Synchronous; the sorts' scratch is allocated on the stream and released. */
int pst_sort_order_by_attribute_device(const pst_buffer* b, const char* name, const pst_datatype* dt, uint32_t component, uint32_t descending,
                                       uint32_t* d_order);
/* d_keys (device, nullable): also the key of point i, len u64 values */
int pst_morton_order_device(const pst_buffer* b, uint32_t dims, uint32_t bits, uint32_t* d_order, uint64_t* d_keys);
int pst_shuffle_order_device(uint64_t n, uint64_t seed, uint32_t* d_order);
/* d_inverse[d_order[j]] = j for j < n; entries >= n are skipped.  Stream-ordered.  The two arrays are different ones. */
int pst_invert_order_device(const uint32_t* d_order, uint64_t n, uint32_t* d_inverse);
/* The gather kernel's seams (tests place their sizes around them; each pointer optional): consecutive output points one workgroup owns, and
 * the bytes of the LDS record tile of the pairings with an interleaved side (records of which fewer than 16 fit it take a plain byte-copy
 * kernel).  Host only. */
int pst_reorder_kernel_shape(uint32_t* points_per_block, uint32_t* record_tile_bytes);
/* Measurement aid.  With PST_REORDER_TIMES=1 in the environment the synchronous calls above bracket their phases with stream events; this
 * returns the calling thread's last such call: ms = {bounds and keys, sort, gather}, a phase the call does not have as 0.  Zeros without the
 * switch.  Host only. */
int pst_reorder_phase_times(double ms[3]);

/* ---- Ground classification (progressive morphological filter) ------------------------------------------------------------------------
 * What PDAL's filters.pmf and PCL's ProgressiveMorphologicalFilter compute (Zhang et al. 2003; the reference has neither), with square
 * windows: the points are rasterised to their lowest z per cell, the raster is opened (eroded, then dilated) with growing windows, and a
 * point is ground when it lies no higher above an opened surface than that window's threshold.  All arithmetic is f64, every operation
 * separately rounded.  The definition:
 *   parameters:  cell_size finite and > 0; max_window_size, slope, initial_distance, max_distance finite and >= 0; base >= 2 when
 *                exponential != 0, >= 1 otherwise.  Anything else -> PST_ERR_INVALID_ARGUMENT.
 *   schedule:    for k = 0, 1, ...: half-width in cells h_k = base^k (exponential) or (k + 1) * base (linear), window w_k = 2 h_k + 1;
 *                threshold th_0 = initial_distance, th_k = min(max_distance, ((slope * (double)(w_k - w_(k-1))) * cell_size) +
 *                initial_distance) (eq. 7 of the paper).  Window k is appended; the schedule ends after the first k with
 *                (double)w_k * cell_size >= max_window_size.  More than 32 windows, or a half-width of 2^30 cells and more ->
 *                PST_ERR_INVALID_ARGUMENT.
 *   finite:      a point whose x, y and z are all finite; every other point is never ground and takes no part.
 *   grid:        (x0, y0) = the smallest x and the smallest y of the finite points; col = (uint32)((x - x0) / cell_size), row likewise
 *                from y; cols, rows = the largest col, row + 1.  cols * rows > 2^28 -> PST_ERR_UNSUPPORTED (use a larger cell).
 *   surface:     Z_0[cell] = the smallest z of the cell's finite points, +inf for an empty cell.  Per window: E_k = erode(Z_k, h_k),
 *                D_k = dilate(E_k, h_k), L = min(L, D_k + th_k) cell by cell (L starts as +inf), Z_(k+1) = D_k.
 *                erode(A, h)[r][c] = the minimum of A over the square |dr| <= h, |dc| <= h clipped to the grid; dilate(A, h)[r][c] = the
 *                maximum over the same square of the entries below +inf, +inf if there is none.
 *   result:      point i is ground iff it is finite and z_i <= L[row_i][col_i].  Values are compared as values (-0.0 == 0.0).
 * Only minima, maxima and one addition per cell and window: the result does not depend on any order of evaluation, and two calls write the
 * same bytes.  Position3D not stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE; interleaved or columnar, owned, sliced or external, at any
 * byte offset.  2^32 - 16 points and more -> PST_ERR_UNSUPPORTED.  Null arguments, invalid parameters and an empty buffer are answered
 * before a device is looked for; without a device every other call is PST_ERR_NO_DEVICE, never a CPU path.
 * Cost: the positions are read twice (raster, classification) and once more for their bounds; every window is four or more passes over a
 * raster of 8-byte cells.  Device scratch: 32 bytes per cell. */
/* The parameters travel as seven scalars (cell_size, max_window_size, slope, initial_distance, max_distance, exponential, base): no struct
 * crosses the boundary.  The schedule of those parameters: *n_windows <= 32 windows, their half-widths in cells and thresholds (each array
 * optional).  Host only. */
int pst_pmf_schedule(double cell_size, double max_window_size, double slope, double initial_distance, double max_distance, int exponential, uint32_t base,
                     uint32_t half_widths[32], double thresholds[32], uint32_t* n_windows);
/* The raster's geometry, so that a caller can size the surfaces: origin = {x0, y0}, dim = {cols, rows}, *n_finite = the finite points.
 * A buffer without a finite point (an empty one is answered on the host): zeros.  Synchronous. */
int pst_pmf_grid(const pst_buffer* b, double cell_size, double origin[2], uint32_t dim[2], uint64_t* n_finite);
/* Synchronous.  mask: len bytes, 1 = ground, in device memory (mask_memkind = PST_MEM_DEVICE) or host memory (anything else), the
 * convention of the outlier masks.  surfaces (nullable; surfaces_memkind likewise): f64 [3][rows][cols] of pst_pmf_grid's dim -- the min-z
 * raster Z_0, the last opened surface, L.  *n_ground = the ones of the mask.  An empty buffer and one without a finite point are answered
 * without a raster: an all-zero mask, *n_ground = 0, the surfaces untouched. */
int pst_pmf_ground_mask(const pst_buffer* b, double cell_size, double max_window_size, double slope, double initial_distance, double max_distance, int exponential, uint32_t base,
                        uint8_t* mask, uint32_t mask_memkind, double* surfaces, uint32_t surfaces_memkind, uint64_t* n_ground);
/* erode (op 0) / dilate (op 1) as defined above of a caller's raster, f64 [rows][cols] in DEVICE memory, by a square of half_width cells:
 * what a terrain-model user opens or closes a surface with.  Entries are finite or +inf (a NaN counts as +inf).  Stream-ordered; NOT in
 * place: d_in and d_out must not overlap.  cols * rows > 2^28 -> PST_ERR_UNSUPPORTED; a raster without cells is answered on the host. */
int pst_grid_morphology_device(const double* d_in, double* d_out, uint32_t cols, uint32_t rows, uint32_t half_width, uint32_t op);
/* d_mask[i] = 1 iff point i is finite as defined above, len bytes in DEVICE memory; stream-ordered.  With the ground mask it gives "finite
 * and not ground", the points a ground removal keeps (pst_buffer_set_u8_where_device on the mask's own buffer clears the ground points). */
int pst_finite_mask_device(const pst_buffer* b, uint8_t* d_mask);
/* The U8 attribute of that name (interleaved or columnar) = value wherever the mask byte of the point, in DEVICE memory, is not zero; the
 * other points keep theirs.  No such U8 attribute -> PST_ERR_MISSING_ATTRIBUTE.  Stream-ordered: how a ground mask becomes LAS class 2. */
int pst_buffer_set_u8_where_device(pst_buffer* b, const char* attribute_name, const uint8_t* d_mask, uint8_t value);
/* The kernels' seams (tests place their sizes around them; each pointer optional): points per workgroup of the raster, classification and
 * set-where passes; columns and rows of the raster tile one workgroup of a morphology pass writes; the largest half-width of one pass (a
 * larger one runs as successive passes whose half-widths add up to it).  Host only. */
int pst_pmf_kernel_shape(uint32_t* points_per_block, uint32_t* tile_cols, uint32_t* tile_rows, uint32_t* max_half_width);
/* Measurement aid.  With PST_PMF_TIMES=1 in the environment pst_pmf_ground_mask brackets its three phases with stream events; this returns
 * the calling thread's last call: ms = {bounds + raster, morphology, classification}.  Zeros without the switch.  Host only. */
int pst_pmf_phase_times(double ms[3]);

/* ---- Nearest neighbours between two clouds, ICP ----------------------------------------------------------------------------------------
 * What CloudCompare's cloud-to-cloud distance, PDAL's filters.icp and PCL's CorrespondenceEstimation / IterativeClosestPoint compute (the
 * reference has none of them): for every point of a QUERY cloud the nearest point of a different TARGET cloud, and on top of it the rigid
 * alignment of one scan to another.  The definitions:
 *   points:       target points are the Position3D (Vec3f64) of the target buffer; query points those of the query buffer, optionally sent
 *                 through a rigid transform T of 12 doubles, row-major [R | t], as they are loaded:
 *                 x' = ((r00*x + r01*y) + r02*z) + t0, y' and z' alike.
 *   distance:     d2(q', p) = (dx*dx + dy*dy) + dz*dz, dx = p.x - q'.x (y, z alike).  Every operation here and above is a separately
 *                 rounded f64 operation (no contraction).
 *   match:        for a finite query, the finite target with the smallest d2 among those with d2 <= m2, m2 = max_distance * max_distance
 *                 rounded once on the host; equal d2 goes to the lower target buffer index.  idx = that buffer index, dist = sqrt(d2).
 *   no match:     idx = 0xFFFFFFFF and dist = +inf: a query that is not finite after the transform, no target within max_distance, an empty
 *                 target, a target without a finite point.  Targets that are not finite are never matched.
 *   max_distance: +inf means unbounded.  NaN, zero, negative, or a value whose square is neither a normal number nor +inf ->
 *                 PST_ERR_INVALID_ARGUMENT.
 * The result is a function of the two clouds, T and max_distance alone: not of the index's cell edge, not of the order in which the search
 * visits cells, not of the storage kind.
 *   ICP step:     the search with T_in; M = the matched source points, m = |M|, o = the grid origin of the index.
 *                 first pass:  cq = o + sum(q' - o) / m, cp = o + sum(p - o) / m
 *                 second pass: H = sum (q' - cq)(p - cp)^T, sum_d2 = sum d2
 *                 Both are fixed-shape reductions in source-buffer order (blocks of a fixed number of points, a fixed tree per block, the
 *                 block partials added in block order by one workgroup; no floating-point atomics): two calls give the same bits.
 *                 sums[17] = {(double)m, cq[3], cp[3], H[9] row-major, sum_d2}.  dR = the proper rotation (orthonormal, determinant +1) that
 *                 maximises trace(dR H) (Horn's unit quaternion; a rank-deficient H still gives a proper rotation), dt = cp - dR cq,
 *                 T_out = (dR | dt) o T_in: R_out = dR R_in, t_out = dR t_in + dt.  rms = sqrt(sum_d2 / m) is the misfit of T_in, not of
 *                 T_out.  m < 3 -> PST_ERR_TOO_FEW_POINTS.
 *   ICP loop:     T_0 = T_init (NULL: the identity); the step is repeated and the loop stops after the step whose rms differs from the
 *                 previous step's by at most rms_tolerance (absolute, in the cloud's units, >= 0), or after max_iterations steps (>= 1).
 *                 It IS the step function called in a loop: the same bits.
 *   normals:      point-to-plane ICP needs a normal per target.  pst_nn_index_set_normals* gathers the normals of the finite targets into
 *                 the index's sorted order, as f64, in a second block of device memory the index owns (24 bytes per finite target).  They
 *                 are used AS GIVEN, neither normalised nor re-oriented: the sign of a normal does not change the step (j and r below both
 *                 change sign, every sum is bit-identical), and a normal that is not of unit length weights its pair by its squared
 *                 length, as in PCL.
 *   plane step:   the search with T_in exactly as in the ICP step; M the matched source points, m = |M|.  A matched pair (q', p, n), n
 *                 the normal of p, is USED when n's three components are finite and (nx*nx + ny*ny) + nz*nz > 0; U = the used pairs,
 *                 u = |U|, o = the grid origin.
 *                 first pass, over U:  cq = o + sum(q' - o) / u, sum_d2 = sum d2, and the counts m and u
 *                 second pass, over U: w = q' - cq;  a = w x n: a0 = w1*n2 - w2*n1, a1 = w2*n0 - w0*n2, a2 = w0*n1 - w1*n0;
 *                                      r = ((p0 - q'0)*n0 + (p1 - q'1)*n1) + (p2 - q'2)*n2;  j = (a0, a1, a2, n0, n1, n2);
 *                                      A[i][k] = sum j_i*j_k (i <= k), g_i = sum j_i*r, sum_r2 = sum r*r,
 *                                      sum_w2 = sum ((w0*w0 + w1*w1) + w2*w2)
 *                 Every operation is a separately rounded f64 operation; both passes are fixed-shape reductions of the form above (the same
 *                 constants, pst_nn_kernel_shape): two calls give the same bits.
 *                 sums[35] = {(double)m, (double)u, cq[3], A[21] (upper triangle, row-major), g[6], sum_r2, sum_w2, sum_d2}.
 *                 The update minimises sum (r - omega.a - tau.n)^2 over a rotation vector omega about cq and a translation tau.  With
 *                 L = sqrt(sum_w2 / u) (1 when that is 0 or not finite), S = diag(1/L, 1/L, 1/L, 1, 1, 1), A' = S A S, g' = S g and the
 *                 eigen-decomposition A' = sum lambda_i v_i v_i^T (cyclic Jacobi): y = sum over lambda_i > 2^-30 * lambda_max of
 *                 v_i (v_i . g') / lambda_i, the minimum-norm solution -- a direction the pairs do not constrain (all normals parallel: three
 *                 of them; a sphere: the rotations; a cylinder: one rotation and one translation) gets NO motion.  2^-30 is a definition.
 *                 lambda_max <= 0 or a non-finite A gives the identity update.  omega = y[0..3] / L, tau = y[3..6], dR = exp([omega]x)
 *                 (Rodrigues; a proper rotation to rounding for any omega), dt = (cq + tau) - dR cq, T_out = (dR | dt) o T_in.
 *                 rms = sqrt(sum_r2 / u) is the point-to-plane misfit of T_in, not of T_out.  u < 6 -> PST_ERR_TOO_FEW_POINTS; an index
 *                 without normals -> PST_ERR_MISSING_ATTRIBUTE, after the argument checks and before a device is looked for.
 *   plane loop:   pst_icp_plane is pst_icp_plane_step in a loop with the stopping rule of the ICP loop on that rms: the same bits.
 * Checks: null arguments and invalid parameters (max_distance as above; a negative, NaN or infinite cell_edge; a transform entry that is
 * not finite; max_iterations == 0; a negative or NaN rms_tolerance) are answered before a device is looked for; then
 * PST_ERR_MISSING_ATTRIBUTE when Position3D is not stored as Vec3f64; then the device (none: PST_ERR_NO_DEVICE, never a CPU path); then the
 * lengths: 2^32 - 16 points and more in either cloud -> PST_ERR_UNSUPPORTED.  Out of device memory is PST_ERR_OUT_OF_MEMORY and the next
 * call works.  Both clouds may be interleaved or columnar, owned, sliced or external; query and target may be the same buffer.
 * Cost: a query tests the targets of the 27 cells around its own and goes on ring by ring only while its best distance exceeds the rings
 * searched.  A query far outside a large target walks ring after ring, up to the whole grid, unless max_distance bounds it. */
typedef struct pst_nn_index pst_nn_index;
/* The persistent index over `target`: a uniform grid over the finite points' AABB, their positions and buffer indices sorted by cell.  It
 * owns device memory of its own (about 36 bytes per finite target; not the scratch pool: pst_release_scratch leaves it alone), does not
 * keep `target` alive and does not read it after this call.  cell_edge > 0: the grid's cell edge (doubled until no axis has more than
 * 2^21 - 1 cells); 0: chosen so that the occupied cells hold between 2 and 16 points on average.  Synchronous. */
int pst_nn_index_create(const pst_buffer* target, double cell_edge, pst_nn_index** out);
int pst_nn_index_destroy(pst_nn_index* index);
/* What the index was built with (each pointer optional; host only): the grid's origin and its final cell edge, cells per axis, the number of
 * finite targets and of occupied cells.  An index without a finite target reports zeros. */
int pst_nn_index_grid(const pst_nn_index* index, double min_and_edge[4], uint32_t dim[3], uint64_t* n_finite, uint64_t* occupied_cells);
/* Synchronous.  d_idx: len(query) x uint32, d_dist: len(query) x f64, both in DEVICE memory; either may be NULL, not both.  transform12:
 * host, NULL = the query points as they are stored. */
int pst_nearest_neighbours_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double max_distance, uint32_t* d_idx,
                                  double* d_dist);
/* keep_far == 0: d_mask[i] = 1 iff d_dist[i] <= threshold; otherwise d_mask[i] = 1 iff NOT d_dist[i] <= threshold (true for an unmatched
 * point).  Both arrays in DEVICE memory, n elements; stream-ordered, no host synchronisation: the mask is what
 * pst_buffer_filter(..., PST_MEM_DEVICE, ...) and pst_buffer_filter_into_async take.  n == 0 is answered PST_OK on the host, before a device
 * is looked for (as pst_cluster_mask_device does): there is nothing to compute. */
int pst_distance_mask_device(const double* d_dist, uint64_t n, double threshold, int keep_far, uint8_t* d_mask);
/* One ICP step (synchronous; all arrays on the host, T_out may be T_in). */
int pst_icp_step(const pst_nn_index* index, const pst_buffer* source, const double T_in[12], double max_distance, double sums[17], double T_out[12]);
/* The ICP loop (synchronous; every step copies its 17 sums to the host).  T_init: NULL = identity.  rms, matched, iterations (each
 * optional): the last step's misfit and number of matched points, the number of steps run. */
int pst_icp(const pst_nn_index* index, const pst_buffer* source, const double* T_init, double max_distance, uint32_t max_iterations, double rms_tolerance,
            double T_out[12], double* rms, uint64_t* matched, uint32_t* iterations);
/* Target normals for point-to-plane ICP; both setters are synchronous, replace what an earlier set left, and do not read their source after
 * they return.  The normals live in device memory of the index's own (24 bytes per finite target; not the scratch pool: pst_release_scratch
 * leaves it alone), freed by pst_nn_index_destroy.  They are used as given: not normalised (a non-unit normal weights its pair), not
 * re-oriented (the sign of a normal does not change the step).  An index without a finite target accepts normals and holds none.
 * Checks: null arguments, then a wrong n / len(b) (PST_ERR_INVALID_ARGUMENT), then a buffer without a Vec3f32 Normal
 * (PST_ERR_MISSING_ATTRIBUTE), all before a device is looked for; then the device.
 * d_normals: DEVICE memory, f64 [n][3] in target-buffer order: what pst_compute_normals_device writes.  n must equal the target's length at
 * pst_nn_index_create.  NULL (n ignored) drops the normals (host only). */
int pst_nn_index_set_normals_device(pst_nn_index* index, const double* d_normals, uint64_t n);
/* The NORMAL attribute (Vec3f32) of `b` -- what pst_compute_normals_into writes -- widened to f64 (exact); b interleaved or columnar, owned, sliced
 * or external, len(b) == the target's length. */
int pst_nn_index_set_normals(pst_nn_index* index, const pst_buffer* b);
/* *out = 1 when a set of normals has been accepted and not dropped since, else 0.  Host only. */
int pst_nn_index_has_normals(const pst_nn_index* index, int* out);
/* One point-to-plane ICP step (synchronous; all arrays on the host, T_out may be T_in).  Argument checks, limits, out-of-memory behaviour
 * and storages are those of pst_icp_step. */
int pst_icp_plane_step(const pst_nn_index* index, const pst_buffer* source, const double T_in[12], double max_distance, double sums[35], double T_out[12]);
/* The point-to-plane loop (synchronous; every step copies its 35 sums to the host), as pst_icp.  rms, used, iterations (each optional): the last
 * step's point-to-plane misfit and number of used pairs, the number of steps run. */
int pst_icp_plane(const pst_nn_index* index, const pst_buffer* source, const double* T_init, double max_distance, uint32_t max_iterations, double rms_tolerance,
                  double T_out[12], double* rms, uint64_t* used, uint32_t* iterations);
/* The kernels' seams (each pointer optional; host only): queries one workgroup of the search kernel owns (one lane each; candidates are read
 * from the index's sorted arrays, none are staged in LDS), threads of the one workgroup that adds the block partials of the ICP sums, source
 * points per block partial. */
int pst_nn_kernel_shape(uint32_t* queries_per_block, uint32_t* reduce_block, uint32_t* reduce_points_per_block);
/* Measurement aid.  With PST_NN_TIMES=1 in the environment pst_nearest_neighbours_device brackets its two phases with stream events; this
 * returns the calling thread's last call: ms = {query keys + sort, search}.  Zeros without the switch.  Host only. */
int pst_nn_phase_times(double ms[2]);

/* ---- M3C2 change detection ---------------------------------------------------------------------------------------------------------------
 * What CloudCompare's M3C2 plugin and py4dgeo compute (Lague, Brodu & Leroux 2013; the reference has neither): for every CORE point the
 * signed distance between two aligned clouds along the local normal, from the points of each cloud inside a cylinder around that normal,
 * and a 95 % level of detection that says whether the distance is significant.  Where cloud-to-cloud distance is unsigned and grows with
 * point spacing and roughness, this tells erosion from deposition and averages the roughness out.  The definitions; every arithmetic
 * operation is a separately rounded f64 operation (no contraction), square roots and divisions correctly rounded:
 *   inputs:       two indices, `reference` (cloud 1) and `compared` (cloud 2); n core points, the Position3D (Vec3f64) of any buffer (often a
 *                 thinned cloud 1); the cylinder's radius R and half-length L = max_depth; min_points; registration_error.
 *   normal:       of core point i.  d_normals given: row i of that array (DEVICE memory, f64 [n][3] in core order: what
 *                 pst_compute_normals_device writes).  d_normals NULL: the normal `reference` holds for the reference point nearest to
 *                 the core point, which is exactly the match of pst_nearest_neighbours_device with unbounded distance and no transform,
 *                 ties as defined there; a `reference` without normals -> PST_ERR_MISSING_ATTRIBUTE.  Then
 *                 nn = (nx*nx + ny*ny) + nz*nz, s = sqrt(nn), u = (nx/s, ny/s, nz/s).  With PST_M3C2_ORIENT_UP u is negated when uz < 0, or
 *                 uz == 0 && uy < 0, or uz == 0 && uy == 0 && ux < 0.
 *   invalid:      a core point that is not finite, that has no nearest point (d_normals NULL and no finite reference point), whose normal
 *                 has a component that is not finite, or whose nn is 0 or not finite.  Its u is reported as three quiet NaNs
 *                 (0x7FF8000000000000).
 *   membership:   a finite point p of a cloud, d = p - c componentwise: t = (dx*ux + dy*uy) + dz*uz, w = (dx - t*ux, dy - t*uy, dz - t*uz),
 *                 r2 = (wx*wx + wy*wy) + wz*wz; p is a member iff fabs(t) <= L && r2 <= R*R (R*R rounded once; both bounds inclusive).
 *   per cloud X:  n_X = the number of members (u32), St_X = sum t, Stt_X = sum (t*t) over the members.  The order of summation is the
 *                 implementation's, a fixed function of the inputs and the two grids (a fixed assignment of candidates to lanes and a
 *                 fixed tree; no floating-point atomics): two calls give the same bits.  The COUNTS do not depend on the grids at all.
 *   outputs:      for a valid core point with n_1 >= min_points && n_2 >= min_points, in this order of operations:
 *                   mean_X = St_X / (double)n_X;  distance = mean_2 - mean_1
 *                   q_X = Stt_X - (St_X*St_X) / (double)n_X;  var_X = (q_X > 0 ? q_X : 0) / (double)(n_X - 1)
 *                   lod = 1.96 * (sqrt(var_1/(double)n_1 + var_2/(double)n_2) + registration_error)
 *                   significant = fabs(distance) > lod
 *                 With min_points == 1 and a count below 2, lod is NaN and significant 0 (the distance is still reported).  For any other
 *                 core point, invalid ones included, distance and lod are NaN and significant is 0.  Counts and sums are always
 *                 reported, 0 for an invalid core point; an index without a finite point gives counts 0.
 * Checks, on the host before a device is looked for: null reference, compared or core; R and L finite and > 0; registration_error finite
 * and >= 0; min_points >= 1; no unknown flag bits; at most 2^32 - 1 core points; at least one output pointer (n_significant counts as one);
 * all PST_ERR_INVALID_ARGUMENT.  Then PST_ERR_MISSING_ATTRIBUTE when the core buffer's Position3D is not stored as Vec3f64, then when
 * d_normals is NULL and `reference` has no normals; then the device (none: PST_ERR_NO_DEVICE, never a CPU path); then 2^32 - 16 core points
 * and more -> PST_ERR_UNSUPPORTED.  Out of device memory is PST_ERR_OUT_OF_MEMORY and the next call works.  The core buffer may be
 * interleaved or columnar, owned, sliced or external.
 * Cost: one wave per core point walks the rows of cells its cylinder can touch in each grid; a core point whose cylinder misses a grid
 * costs no search there.  A cylinder as long as a whole large grid tests every row of it. */
#define PST_M3C2_ORIENT_UP 1u
/* Synchronous.  Device outputs, each optional: d_distance, d_lod f64 [n]; d_significant u8 [n]; d_counts u32 [n][2] = {n_1, n_2};
 * d_sums f64 [n][4] = {St_1, Stt_1, St_2, Stt_2}; d_unit_normals f64 [n][3] = the u used.  n_significant (host, optional): the number of
 * significant core points.  At least one of the seven must be given. */
int pst_m3c2_device(const pst_nn_index* reference, const pst_nn_index* compared, const pst_buffer* core, const double* d_normals, double radius, double max_depth,
                    uint32_t min_points, double registration_error, uint32_t flags, double* d_distance, double* d_lod, uint8_t* d_significant, uint32_t* d_counts,
                    double* d_sums, double* d_unit_normals, uint64_t* n_significant);
/* The kernel's seams (each pointer optional; host only): core points one workgroup owns, lanes that share one core point (a whole wave:
 * they search the rows of its cylinder in parallel and test the candidates across lanes). */
int pst_m3c2_kernel_shape(uint32_t* cores_per_block, uint32_t* lanes_per_core);
/* Measurement aid.  With PST_M3C2_TIMES=1 in the environment pst_m3c2_device brackets its three phases with stream events; this returns the
 * calling thread's last call: ms = {normal lookup, core keys + sort, cylinder pass}.  Zeros without the switch.  Host only. */
int pst_m3c2_phase_times(double ms[3]);
/* Measurement aid.  With PST_M3C2_WORK=1 in the environment the cylinder pass counts its work (a second instantiation of the kernel: the
 * counters cost nothing when the switch is off); this returns the calling thread's last call: out = {rows of cells searched, candidates
 * tested, members}, over both clouds.  Zeros without the switch.  Host only. */
int pst_m3c2_work(uint64_t out[3]);

/* ---- Height above ground -----------------------------------------------------------------------------------------------------------------
 * What PDAL's filters.hag_nn and lidR's normalize_height(knnidw()) compute (the reference has neither): for every point of a QUERY cloud
 * the elevation of the ground under it, interpolated from its k nearest GROUND points IN THE XY PLANE with inverse squared distance
 * weights, and the point's height above it.  The definitions:
 *   ground set:   G = the points of the `ground` buffer whose Position3D (Vec3f64) has three finite components and whose mask byte is not
 *                 zero; a NULL mask means every point of the buffer.  Points of `ground` that are not finite or not masked are never
 *                 neighbours.
 *   queries:      every point of the `query` buffer; `query` and `ground` may be the same buffer.  A query is finite when its three
 *                 components are.
 *   distance:     d2(q, p) = dx*dx + dy*dy, dx = p.x - q.x, dy = p.y - q.y: z takes no part.  Every operation here and below is a
 *                 separately rounded f64 operation (no contraction); no square root appears anywhere.
 *   neighbours:   of a finite query, the at most k members of G with the lexicographically smallest (d2, ground-buffer index) among those
 *                 with d2 <= m2, m2 = max_distance * max_distance rounded once on the host (+inf: unbounded); in that order
 *                 (d2_0, z_0), ..., (d2_{j-1}, z_{j-1}), 0 <= j <= k.  A query that is not finite has none.
 *   elevation:    w_i = 1.0 / d2_i (inverse SQUARED distance, as in filters.hag_nn).  If w_0 is not below +inf -- d2_0 is 0, or so small
 *                 that its reciprocal overflows -- the query has an exact hit and zg = z_0.  Otherwise num = w_0*z_0, then
 *                 num = num + w_i*z_i for i = 1 .. j-1 in that order; den = w_0, then den = den + w_i in that order; zg = num / den.
 *                 Nothing else is special-cased: what IEEE arithmetic gives is the definition (a neighbour at d2 = +inf of an unbounded
 *                 search has weight 0, and a query all of whose neighbours have gets 0 / 0).
 *   results:      ground_z[i] = zg, hag[i] = q.z - zg.  j = 0 gives NaN in both: no ground within max_distance, an empty or all-masked-out
 *                 G, a query that is not finite.
 *   same buffer:  there is no special case for queries that are themselves ground: with query == ground a ground point finds itself at
 *                 d2 = 0 and gets hag = +0.0 -- EXCEPT when a lower-indexed member of G shares its x and y: that one is the exact hit, and
 *                 the point gets its height over it.
 *   max_distance: validated exactly as pst_nearest_neighbours_device validates it.
 * The result is a function of the two clouds, the mask, k and max_distance alone: not of the grid, not of the order in which the search
 * visits cells, not of the storage kind.
 * Checks: null arguments and invalid parameters (k == 0 or k > max_k = 32; max_distance; a negative, NaN or infinite cell_edge; d_hag and
 * d_ground_z both NULL) are answered before a device is looked for; then PST_ERR_MISSING_ATTRIBUTE when Position3D is not stored as Vec3f64
 * in either buffer; an empty `query` is then PST_OK on the host with nothing written and zeros in the counts and the grid; then the device
 * (none: PST_ERR_NO_DEVICE, never a CPU path); then the lengths: 2^32 - 16 points and more in either buffer -> PST_ERR_UNSUPPORTED.  Out of
 * device memory is PST_ERR_OUT_OF_MEMORY and the next call works.  An empty or all-masked `ground` writes NaN everywhere, sets n_unresolved
 * to the number of finite queries and reports a zero grid.
 * Synchronous (the host reads G's bounds to size the grid).  The index -- G sorted into a uniform XY grid over its AABB with a dense cell
 * directory, 4 bytes per cell -- is rebuilt by every call in the call's scratch.  cell_edge > 0: the grid's cell edge; 0: chosen so that
 * the 3 x 3 cells around a query hold about 2k ground points if G filled its rectangle.  Either is doubled until no axis has more than
 * 2^21 - 1 cells and the grid no more than 2^26.  d_hag, d_ground_z: DEVICE memory, len(query) x f64, either may be NULL, not both.
 * d_ground_mask: DEVICE memory, len(ground) bytes, or NULL.  n_ground = |G|, n_unresolved = the finite queries with j == 0,
 * grid_min_and_edge = {min x, min y, final cell edge} and grid_dim = {columns, rows} of the grid that was used: each optional, host.
 * Cost: a query tests the ground points of the 3 x 3 cells around its own and goes on ring by ring only while its k-th best distance
 * exceeds the rings searched; ring r costs O(r) directory reads.  max_distance bounds the walk. */
int pst_height_above_ground_device(const pst_buffer* query, const pst_buffer* ground, const uint8_t* d_ground_mask, uint32_t k, double max_distance, double cell_edge,
                                   double* d_hag, double* d_ground_z, uint64_t* n_ground, uint64_t* n_unresolved, double grid_min_and_edge[3], uint32_t grid_dim[2]);
/* The inverse of pst_buffer_set_u8_where_device: d_mask[i] = 1 iff the U8 attribute of point i equals `value`, else 0 (DEVICE memory,
 * len(b) bytes).  Stream-ordered, no host synchronisation: how Classification == 2 becomes a ground mask without a host round trip.  An
 * attribute the layout does not have as U8 is PST_ERR_MISSING_ATTRIBUTE; an empty buffer is PST_OK on the host. */
int pst_buffer_u8_equals_mask_device(const pst_buffer* b, const char* attribute_name, uint8_t value, uint8_t* d_mask);
/* The kernels' seams (each pointer optional; host only): queries one workgroup of the search kernel owns (one lane each), the largest k,
 * ground points per block partial of the masked bounds. */
int pst_hag_kernel_shape(uint32_t* queries_per_block, uint32_t* max_k, uint32_t* bounds_points_per_block);
/* Measurement aid.  With PST_HAG_TIMES=1 in the environment pst_height_above_ground_device brackets its three phases with stream events;
 * this returns the calling thread's last call: ms = {ground bounds + keys + sort + directory, query keys + sort, search}.  Zeros without the
 * switch.  Host only. */
int pst_hag_phase_times(double ms[3]);

/* ---- Individual trees: tops by a local-maximum filter, crowns after Silva et al. 2016 -----------------------------------------------------
 * What lidR's locate_trees(lmf(ws, hmin)) and segment_trees(silva2016()) and PDAL's filters.litree are for (the reference has neither):
 * which points are tree tops, and which tree every point belongs to.  Every arithmetic operation below is a separately rounded f64
 * operation (no contraction); no square root appears anywhere.  The definitions:
 *   height:       h_i = the z of point i's Position3D (Vec3f64), or d_heights[i] when that column is given: DEVICE memory, len x f64 -- how
 *                 the d_hag of pst_height_above_ground_device is fed in.  x and y come from the position; z is not consulted when
 *                 d_heights is given.
 *   valid:        x, y and h are finite and d_mask is NULL or d_mask[i] != 0 (DEVICE memory, len bytes).
 *   candidates:   C = the valid points with h_i >= min_height (finite).
 *   window:       window = {a, b, r_min, r_max}, RADII: r_i = min(max(a + b*h_i, r_min), r_max); a, b finite, 0 <= r_min <= r_max, r_min
 *                 finite, r_max may be +inf.  (lidR's ws is a diameter.)  A fixed window is b = 0.  j is in i's window iff
 *                 dx*dx + dy*dy <= r_i*r_i, inclusive, dx = x_j - x_i, dy = y_j - y_i.
 *   dominates:    j dominates i iff h_j > h_i, or h_j == h_i and j < i in buffer order (-0.0 == +0.0).
 *   tops:         candidate i is a tree top iff no OTHER candidate in i's window dominates it.  The window is i's own: with b != 0 the
 *                 relation is deliberately asymmetric, as in lidR.  Points below min_height dominate nobody.  With r_i == 0 the window
 *                 still holds the exact duplicates of i in x and y.
 *   numbering:    the trees are the tops numbered 0 .. n_trees - 1 by descending height, ties (-0.0 and +0.0 tie) by ascending buffer
 *                 index: tallest first, so that pst_cluster_mask_device(first, count) selects the tallest trees.
 *   crowns:       parameters max_crown_factor >= 0 (finite; the crown DIAMETER as a share of the tree's height), exclusion in [0, 1],
 *                 min_height.  The trees T are the VALID points with a non-zero byte in d_top_mask, whatever their height (a caller may
 *                 edit the mask), numbered as above, H_t their heights.  For every valid point p with h_p >= min_height: t = the tree of
 *                 lexicographically smallest (d2, buffer index of the top), d2 as above from p to the top; rc = (0.5*max_crown_factor) * H_t;
 *                 tree_id[p] = the number of t iff d2 <= rc*rc && h_p >= exclusion*H_t, else 0xFFFFFFFF.  The NEAREST top is chosen
 *                 first and then tested, as lidR does -- not the nearest among those that pass.  Every other point gets 0xFFFFFFFF.
 *                 counts[t] = the points labelled t, n_labelled their sum.
 * Both results are functions of the cloud, the heights, the masks and the parameters alone: not of the grid, not of the storage kind; two
 * calls write the same bytes.
 * Checks: null arguments and invalid parameters (min_height not finite; the window's conditions above; max_crown_factor; exclusion; a
 * negative, NaN or infinite cell_edge) are answered before a device is looked for; then PST_ERR_MISSING_ATTRIBUTE when Position3D is not
 * stored as Vec3f64; an empty buffer is then PST_OK on the host with nothing written and zeros in the counts and the grid; then the device
 * (none: PST_ERR_NO_DEVICE, never a CPU path); then 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED.  Out of device memory is
 * PST_ERR_OUT_OF_MEMORY and the next call works.
 * Synchronous.  d_top_mask: DEVICE memory, len bytes, 1 for a top and 0 for every other point: what pst_buffer_filter_into and
 * pst_segment_trees_device take.  d_top_indices (DEVICE, u32, optional): the buffer indices of the tops IN TREE-NUMBER ORDER when they fit
 * `capacity`; more tops than that -> PST_ERR_RANGE with the mask written and the counts set (the pst_plane_inliers convention).
 * n_candidates = |C|, n_tops, grid_min_and_edge = {min x, min y, final cell edge} and grid_dim = {columns, rows} of the candidate grid that
 * was used: each optional, host.  No candidate: an all-zero mask, zero counts, a zero grid.  cell_edge > 0: the grid's cell edge; 0:
 * automatic (half the radius of a window at half the largest |h|, not below a sparse-cloud floor).  Either is doubled until no axis has
 * more than 2^21 - 1 cells and the grid no more than 2^26.
 * Cost: a candidate first tests the candidates of the 3 x 3 cells around it, which decides nearly every point of a canopy; the others, the
 * tops among them, get one wave each for the rest of their window. */
int pst_tree_tops_device(const pst_buffer* b, const double* d_heights, const uint8_t* d_mask, double min_height, const double window[4], double cell_edge,
                         uint8_t* d_top_mask, uint32_t* d_top_indices, size_t capacity, uint64_t* n_candidates, uint64_t* n_tops, double grid_min_and_edge[3],
                         uint32_t grid_dim[2]);
/* Synchronous.  d_tree_id: DEVICE memory, len x u32, the labels (what pst_cluster_mask_device and pst_buffer_set_u8_from_ids_device take).
 * d_tree_counts (DEVICE, u32, optional): counts[t] when the trees fit counts_capacity; more trees than that -> PST_ERR_RANGE with the
 * labels written and *n_trees, *n_labelled set.  No tree: every label 0xFFFFFFFF.  The search is bounded by
 * rc_max = (0.5*max_crown_factor) * max |H|: a top farther away fails its own test.  cell_edge: of the grid over the tops, as above. */
int pst_segment_trees_device(const pst_buffer* b, const double* d_heights, const uint8_t* d_mask, const uint8_t* d_top_mask, double min_height, double max_crown_factor,
                             double exclusion, double cell_edge, uint32_t* d_tree_id, uint32_t* d_tree_counts, size_t counts_capacity, uint64_t* n_trees,
                             uint64_t* n_labelled);
/* The kernels' seams (each pointer optional; host only): candidates one workgroup of the near pass owns (one lane each), survivors one
 * workgroup of the far pass owns (one wave each), queries one workgroup of the crown search owns, points per block partial of the member
 * pass. */
int pst_trees_kernel_shape(uint32_t* points_per_block, uint32_t* survivors_per_block, uint32_t* queries_per_block, uint32_t* bounds_points_per_block);
/* Measurement aid.  With PST_TREES_TIMES=1 in the environment both calls bracket their phases with stream events; this returns the calling
 * thread's last call: ms = {candidate index, local-maximum filter, numbering, top index + crown search}; pst_tree_tops_device leaves the
 * last one 0, pst_segment_trees_device the first two.  Zeros without the switch.  Host only. */
int pst_trees_phase_times(double ms[4]);
/* Measurement aid: out = {candidates, candidates the near pass left undecided, candidates the far pass tested} of the calling thread's last
 * pst_tree_tops_device; the last one is counted only with PST_TREES_WORK=1 in the environment (a second instantiation of the kernel), else
 * 0.  Host only. */
int pst_trees_work(uint64_t out[3]);

/* ---- Rasterisation: per-cell statistics of a cloud on an XY grid -------------------------------------------------------------------------
 * What PDAL's writers.gdal computes before it writes a file (the reference has nothing like it): a surface model (MAX of z), a canopy height
 * model (MAX of the height above ground), a density image (COUNT), an intensity image (MEAN), and the hole filler every such raster
 * needs.  Every operation below is a separately rounded f64 operation (no contraction); no square root appears anywhere.  The definitions:
 *   value:       v_i = the z of point i (d_values == NULL), or d_values[i]: DEVICE memory, len x f64 -- how the d_hag of
 *                pst_height_above_ground_device is rasterised.  z is not consulted when d_values is given.
 *   grid:        origin = {x0, y0} and dim = {cols, rows} both given: the caller's grid.  Both NULL: exactly the grid
 *                pst_pmf_grid(b, cell_size) reports -- over the points with three finite components, WHATEVER d_mask says, so the rasters
 *                of different masks of one cloud line up cell for cell (a zero origin may differ in its sign).  One without the other, a
 *                zero in a given dim, an origin that is not finite, a cell_size that is not finite and positive -> PST_ERR_INVALID_ARGUMENT;
 *                cols * rows > 2^28 -> PST_ERR_UNSUPPORTED.
 *   cell:        qx = (x - x0) / cell_size, qy = (y - y0) / cell_size.  The point is inside iff qx >= 0.0 && qx < (double)cols &&
 *                qy >= 0.0 && qy < (double)rows, compared as doubles; then col = (uint32)qx, row = (uint32)qy.  A point exactly at x0 is
 *                in, one at x0 + cols * cell_size is out, and so is one below x0 by one ulp (a negative quotient).  No finite point is
 *                outside the automatic grid.
 *   member:      point i is a member iff x and y are finite, v_i is finite, d_mask is NULL or d_mask[i] != 0 (DEVICE memory, len bytes),
 *                and the point is inside.
 *   statistics:  `stats` is a set of PST_RASTER_COUNT (1), PST_RASTER_MIN (2), PST_RASTER_MAX (4), PST_RASTER_MEAN (8) and
 *                PST_RASTER_VARIANCE (16); 0 or a value above 31 -> PST_ERR_INVALID_ARGUMENT.  out = f64 [planes][rows][cols], one plane per
 *                set bit in ascending bit order, in device memory (out_memkind = PST_MEM_DEVICE) or host memory (anything else), the
 *                convention of pst_pmf_ground_mask's surfaces.  Per cell, with its members v_0 .. v_(m-1) in ascending buffer index:
 *                  COUNT     (double)m
 *                  MIN, MAX  the member value that is smallest / largest with -0.0 below +0.0; the bits are a member's bits
 *                  MEAN      S / (double)m, S the CHUNKED sum of the v_t, as is every sum here: chunk j holds the members
 *                            [256 j, min(m, 256 (j + 1))) (PST_RASTER_CHUNK = 256 is part of this definition), P_j is its left-to-right
 *                            sum starting from its first element, and S = P_0 + P_1 + ... left to right
 *                  VARIANCE  SS / (double)m (the population variance): d_t = v_t - MEAN, SS the same chunked sum of the d_t * d_t
 *                An empty cell has COUNT +0.0 and the canonical quiet NaN (0x7FF8000000000000) in every other plane.  Beyond this, what
 *                IEEE arithmetic gives is the definition (a sum that overflows, for example).
 *   results:     *n_members = the sum of the counts; origin_out, dim_out (each optional) = the grid that was used.
 * The result is a function of the points in buffer order, the values, the mask, the grid and `stats` alone, and two calls write the same
 * bytes: COUNT, MIN and MAX do not depend on any order, and the sums have the one above.  The chunks exist so that a cell need not be summed
 * end to end: a request for COUNT, MIN and MAX alone takes one pass of atomics over the positions and no sort; any other sorts the points by
 * cell with the library's stable radix sort and walks every cell in buffer order, a cell of more than one chunk with a workgroup of its own.
 * Checks, in the order of pst_pmf_ground_mask: null arguments (b, out, n_members) and invalid parameters are answered before a device is
 * looked for; then PST_ERR_MISSING_ATTRIBUTE when Position3D is not stored as Vec3f64; an empty buffer with the automatic grid is PST_OK on
 * the host with a zero geometry and nothing written (with a given grid `out` is still filled with the empty-cell values, which needs the
 * device); then the device (none: PST_ERR_NO_DEVICE, never a CPU path); then 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED.  A buffer
 * without a finite point and with the automatic grid: a zero geometry, *n_members = 0, `out` untouched.  Out of device memory is
 * PST_ERR_OUT_OF_MEMORY and the next call works.  Synchronous.  Interleaved or columnar, owned, sliced or external, at any byte offset.
 * Device scratch: up to 20 bytes per cell on the atomic path; 24 bytes per point and 4 per cell on the sorted one. */
enum {
  PST_RASTER_COUNT = 1,
  PST_RASTER_MIN = 2,
  PST_RASTER_MAX = 4,
  PST_RASTER_MEAN = 8,
  PST_RASTER_VARIANCE = 16,
  PST_RASTER_CHUNK = 256
};
int pst_rasterize(const pst_buffer* b, const double* d_values, const uint8_t* d_mask, double cell_size, const double origin[2], const uint32_t dim[2], uint32_t stats,
                  double* out, uint32_t out_memkind, double origin_out[2], uint32_t dim_out[2], uint64_t* n_members);
/* The hole filler (writers.gdal's window_size) of a caller's raster, f64 [rows][cols] in DEVICE memory.  An entry is EMPTY when it is not
 * finite: the NaN of pst_rasterize and the +inf of the ground filter's surfaces alike.  out[r][c] = in[r][c], the same bits, where the
 * entry is not empty.  Otherwise the cells (r + dr, c + dc) with |dr| <= half_width and |dc| <= half_width that are inside the raster and
 * not empty are visited in row-major order (dr ascending, then dc ascending) with w = 1.0 / (double)(dr*dr + dc*dc): the first one sets
 * num = w*v, den = w, every later one num = num + w*v, den = den + w, and out = num / den -- the canonical NaN if none was visited.
 * half_width 0 copies the raster bit for bit, its empty entries included.  half_width > 16 -> PST_ERR_INVALID_ARGUMENT (an inverse-distance
 * fill does not compose from smaller ones).  Stream-ordered; NOT in place (d_in == d_out -> PST_ERR_INVALID_ARGUMENT; the two must not
 * overlap).  cols * rows > 2^28 -> PST_ERR_UNSUPPORTED; a raster without cells is answered on the host. */
int pst_grid_fill_device(const double* d_in, double* d_out, uint32_t cols, uint32_t rows, uint32_t half_width);
/* The kernels' seams (each pointer optional; host only): points per workgroup of the atomic pass, the chunk length of the sums
 * (PST_RASTER_CHUNK), columns and rows of the raster tile one workgroup of the fill writes, the largest half-width of the fill. */
int pst_raster_kernel_shape(uint32_t* points_per_block, uint32_t* chunk, uint32_t* fill_tile_cols, uint32_t* fill_tile_rows, uint32_t* fill_max_half_width);
/* Measurement aid.  With PST_RASTER_TIMES=1 in the environment pst_rasterize brackets its three phases with stream events; this returns the
 * calling thread's last call: ms = {bounds (zero with a given grid), keys + sort + directory (zero on the atomic path), reduction +
 * output}.  Zeros without the switch.  Host only. */
int pst_raster_phase_times(double ms[3]);

/* ---- Geometric features: the eigenvalues of the neighbourhood covariance and what is derived from them -----------------------------------
 * What PDAL's filters.covariancefeatures / filters.eigenvalues, CloudCompare's "geometric features" and jakteristics compute (the reference
 * has none of it): per point the three eigenvalues of the covariance of its k nearest neighbours, linearity, planarity, scattering,
 * anisotropy, surface variation, omnivariance, eigenentropy, verticality, and the normal, oriented upwards.  Every operation below is a
 * separately rounded f64 operation; the only exceptions are cbrt and log.  tests/features_ref.py restates the definition in numpy.
 *   inputs:        Position3D stored as Vec3f64 (interleaved or columnar, owned, sliced or external, at any byte offset); k; neighbour lists
 *                  uint32 [n][k] in device memory; max_distance (+inf: no limit; a NaN or a negative value -> PST_ERR_INVALID_ARGUMENT); a
 *                  set of PST_FEATURE_* bits (0 or a value above 8191 -> PST_ERR_INVALID_ARGUMENT).
 *   neighbourhood: the slots t = 0 .. k-1 of query q are taken in slot order; the lists need not be sorted.  Slot t with index j is VALID
 *                  iff j < n (the 0xFFFFFFFF padding and any out-of-range index are skipped and never dereferenced), the three coordinates
 *                  of p_j are finite, and d <= max_distance with d = sqrt((dx*dx + dy*dy) + dz*dz), dx = p_j.x - q.x (y, z alike): the
 *                  slot distance of pst_knn_search_device.  A query with a coordinate that is not finite has no valid slot.  The query
 *                  itself counts when its list names it (slot 0 of the library's own lists).  m = the number of valid slots.
 *   centroid:      each component summed over the valid slots left to right, starting from the first valid one, then / (double)m.
 *   covariance:    d = p - c; the six sums of d_a * d_b left to right the same way, then / (double)m (the population covariance, as
 *                  PST_RASTER_VARIANCE is).
 *   eigen-solve:   scale = the largest absolute value of the six entries.  m < 3, or scale not finite: every requested plane but COUNT, and
 *                  both vectors, are the canonical quiet NaN (0x7FF8000000000000).  scale == 0: the eigenvalues are +0.0 and V = I.
 *                  Otherwise A = C / scale entry by entry, V = I, and cyclic Jacobi, at most 10 sweeps.  A sweep first stops the iteration
 *                  if a01 == 0 && a02 == 0 && a12 == 0; then it visits (p, q) = (0, 1), (0, 2), (1, 2), r the third index:
 *                    g = |a_pq|; if g != 0 && |a_pp| + g == |a_pp| && |a_qq| + g == |a_qq| then a_pq = 0;  if a_pq == 0: next pair;
 *                    theta = (a_qq - a_pp) / (2.0 * a_pq);  t = (theta < 0 ? -1.0 : 1.0) / (|theta| + sqrt(theta * theta + 1.0));
 *                    c = 1.0 / sqrt(t * t + 1.0);  s = t * c;  and from the old values
 *                    a_pp' = a_pp - t * a_pq, a_qq' = a_qq + t * a_pq, a_pq' = 0, a_rp' = c * a_rp - s * a_rq, a_rq' = s * a_rp + c * a_rq,
 *                    and for each row i of V: v_ip' = c * v_ip - s * v_iq, v_iq' = s * v_ip + c * v_iq.
 *                  After the sweeps lambda_i = a_ii * scale; the diagonal is the answer even if the cap was reached.
 *   order:         the eigenvalues sorted descending, stably (equal values: the lower original index first), each then clamped
 *                  (lambda > 0 ? lambda : +0.0): l1 >= l2 >= l3 with the eigenvector columns e1, e2, e3 of V.  A vector is negated
 *                  (unary minus of each component) iff z < 0, or z == 0 && y < 0, or z == 0 && y == 0 && x < 0: normals point up.
 *   planes:        out = f64 [planes][n] in device memory, one plane per set bit in ascending bit order.  S = (l1 + l2) + l3, e_i = l_i / S:
 *                    EIGENVALUE_1, _2, _3   l1, l2, l3             SURFACE_VARIATION  l3 / S
 *                    LINEARITY              (l1 - l2) / l1         EIGENVALUE_SUM     S
 *                    PLANARITY              (l2 - l3) / l1         VERTICALITY        1.0 - |e3.z|
 *                    SCATTERING             l3 / l1                OMNIVARIANCE       cbrt((e_1 * e_2) * e_3)
 *                    ANISOTROPY             (l1 - l3) / l1         EIGENENTROPY       h = 0; for i = 1, 2, 3 with e_i > 0: h = h - e_i * log(e_i)
 *                    COUNT                  (double)m, always written
 *                  l1 == 0 (coincident points): the eigenvalue planes and the sum are +0.0; every ratio, verticality, omnivariance, the
 *                  entropy and both vectors are the canonical NaN, written explicitly.
 *   vectors:       d_normals f64 [n][3] (e3) and d_directions f64 [n][3] (e1), device memory, each nullable; at least one of d_out,
 *                  d_normals and d_directions must be given (else PST_ERR_INVALID_ARGUMENT). */
enum {
  PST_FEATURE_EIGENVALUE_1 = 1,
  PST_FEATURE_EIGENVALUE_2 = 2,
  PST_FEATURE_EIGENVALUE_3 = 4,
  PST_FEATURE_LINEARITY = 8,
  PST_FEATURE_PLANARITY = 16,
  PST_FEATURE_SCATTERING = 32,
  PST_FEATURE_ANISOTROPY = 64,
  PST_FEATURE_SURFACE_VARIATION = 128,
  PST_FEATURE_EIGENVALUE_SUM = 256,
  PST_FEATURE_VERTICALITY = 512,
  PST_FEATURE_OMNIVARIANCE = 1024,
  PST_FEATURE_EIGENENTROPY = 2048,
  PST_FEATURE_COUNT = 4096,
  PST_FEATURE_ALL = 8191
};
/* The kernel alone, over a caller's lists d_knn (device, uint32 [n][k], required), k = 1 .. 64 (else PST_ERR_INVALID_ARGUMENT).
 * Stream-ordered on the current stream: no host synchronisation, no allocation.  Checks: null arguments and invalid parameters, then
 * PST_ERR_MISSING_ATTRIBUTE when Position3D is not stored as Vec3f64, all before a device is looked for; an empty buffer is PST_OK on the
 * host; then the device (none: PST_ERR_NO_DEVICE, never a CPU path); then 2^32 - 16 points and more -> PST_ERR_UNSUPPORTED. */
int pst_geometric_features_from_knn_device(const pst_buffer* b, size_t k, const uint32_t* d_knn, double max_distance, uint32_t features, double* d_out,
                                           double* d_normals, double* d_directions);
/* The search of pst_knn_search_device (the same lists, checks and limits: k = 3 .. 64, at least 3 points, fewer than 2^32 - 16, Vec3f64),
 * then the kernel above, then a synchronisation.  d_knn (device, nullable): also receive the lists, uint32 [n][k]; scratch otherwise. */
int pst_geometric_features(const pst_buffer* b, size_t k, double max_distance, uint32_t features, double* d_out, double* d_normals, double* d_directions,
                           uint32_t* d_knn);
/* The kernel's seams for this k (tests place their sizes around them; each pointer optional): points whose whole neighbour lists one
 * workgroup owns, and its threads.  k outside 1 .. 64 -> PST_ERR_INVALID_ARGUMENT.  Host only. */
int pst_features_kernel_shape(size_t k, uint32_t* points_per_block, uint32_t* threads);

/* ---- Polygon crop and overlay: point-in-polygon ids and masks ---------------------------------------------------------------------------
 * What PDAL's filters.crop (polygon, inside or outside) and filters.overlay, and lidR's clip_roi and merge_spatial compute (the reference has
 * neither): which polygon of a set a point falls in.  The definition, which both kernels and tests/crop_ref.py evaluate exactly:
 *   polygon set:  P >= 1 polygons; a polygon is one or more rings; a ring is at least 3 vertices (x, y) in f64, all finite, closed
 *                 implicitly, last vertex to first (a repeated first vertex is allowed and adds only a degenerate edge).  Ring orientation
 *                 carries no meaning: holes, islands inside holes and self-intersections are all handled by the even-odd rule.
 *   edges:        an edge with a.y == b.y is dropped; every other edge is stored canonically, lo = the endpoint with the smaller y, hi = the
 *                 other (an "entry").
 *   crossing:     a point p with finite p.x and p.y crosses an entry iff lo.y <= p.y and p.y < hi.y and d > 0, where
 *                 d = (hi.x - lo.x) * (p.y - lo.y) - (p.x - lo.x) * (hi.y - lo.y), evaluated in f64 with one rounding per operation (four
 *                 subtractions, two products, one subtraction; no FMA).  An infinite or NaN d gives "d > 0" false.  z is ignored, even
 *                 when it is not finite.
 *   containment:  p is in a polygon iff it crosses an odd number of that polygon's entries; a point whose x or y is not finite is in no
 *                 polygon.  id = the smallest polygon index that contains p, or 0xFFFFFFFF (no polygon).  mask = (id != 0xFFFFFFFF); with
 *                 `outside` the byte-for-byte complement, so an outside crop keeps the points that are not finite.
 * Consequences: containment is half-open like the raster's cells (of the unit square the left and bottom edges are inside, the right and top
 * edges outside); two polygons that share an edge evaluate the identical expression for it, whatever direction each ring runs it, so the XOR
 * of the containments of the cells of a subdivision is the containment of its outline, exactly; for a vertical edge d is
 * -(p.x - lo.x) * (hi.y - lo.y), whose sign is exact, so axis-aligned rectangles that tile a grid give every point to exactly the cell that
 * comparisons against the grid lines give.
 * The result is a function of the set and the points alone: not of the kernel, the number of bands or the storage kind.  Two kernels, one
 * launch per query: "flat" keeps every entry in LDS and serves sets of at most pst_crop_kernel_shape's flat_max_edges
 * entries; "banded" walks, per point, the list of the y-band the point is in.  The band directory is built on the host: B equal bands over
 * the box's [ymin, ymax]; band(y) = clamp(floor((y - ymin) * scale), 0, B - 1), scale = B / (ymax - ymin) rounded once; an entry is listed in
 * the bands band(lo.y) .. band(hi.y).  Every step of band() is monotone in y, so a point's band lists every entry it can cross, without
 * any epsilon.
 * Checks: null arguments and an invalid set are answered before a device is looked for; then PST_ERR_MISSING_ATTRIBUTE when Position3D is not
 * stored as Vec3f64; an empty buffer is answered on the host; then the device (none: PST_ERR_NO_DEVICE, never a CPU path); 2^32 - 16 points
 * and more -> PST_ERR_UNSUPPORTED.  Interleaved or columnar, owned, sliced or external, the position at any byte offset.
 * Cost per point and entry tested: 7 f64 operations and 3 compares; traffic: the 24-byte positions in (z rides along in the same lines),
 * 1 or 4 bytes out. */
typedef struct pst_polygon_set pst_polygon_set;
/* The set, indexed on the host and copied into device memory of its own (36 bytes per entry or directory entry; not the scratch pool).  xy:
 * the vertices, x and y interleaved, ring after ring; ring r = vertices ring_offsets[r] .. ring_offsets[r + 1] - 1 (n_rings + 1 offsets, from
 * 0).  polygon_of_ring: n_rings polygon indices, not decreasing from 0 without gaps; NULL = one polygon made of all rings.  bands: B, 0 =
 * chosen from the number of entries.  kernel: 0 = automatic (flat up to flat_max_edges entries), 1 = flat, 2 = banded.  The caller's arrays
 * are not read after the call.  PST_ERR_INVALID_ARGUMENT, with the limit named in the message: a ring of fewer than 3 vertices, offsets that
 * do not start at 0 or decrease, a vertex that is not finite, a polygon_of_ring with a gap, more than 2^24 vertices, more than 2^24 bands,
 * more than 2^27 directory entries (entries summed over the bands that list them: ask for fewer bands), kernel > 2, flat asked for a set of
 * more than flat_max_edges entries.  Synchronous. */
int pst_polygon_set_create(const double* xy, const uint64_t* ring_offsets, size_t n_rings, const uint32_t* polygon_of_ring, uint32_t bands, uint32_t kernel,
                           pst_polygon_set** out);
int pst_polygon_set_destroy(pst_polygon_set* set);
/* What the set was built with (each pointer optional; host only): counts = {polygons, entries, bands, directory entries}, box = {xmin, ymin,
 * xmax, ymax} over all vertices, *kernel = the kernel taken (1 flat, 2 banded). */
int pst_polygon_set_info(const pst_polygon_set* set, uint64_t counts[4], double box[4], uint32_t* kernel);
/* d_ids[i] = the id of point i as defined above: len x uint32 in DEVICE memory.  Stream-ordered on the thread's current stream, nothing is
 * read back: it can be captured in a graph. */
int pst_points_in_polygons_device(const pst_polygon_set* set, const pst_buffer* b, uint32_t* d_ids);
/* d_mask[i] = the mask byte of point i as defined above (outside != 0: the complement): len bytes in DEVICE memory, what
 * pst_buffer_filter(..., PST_MEM_DEVICE, ...), pst_buffer_filter_into and pst_buffer_filter_into_async take.  count == NULL: stream-ordered,
 * nothing is read back.  Otherwise *count = the ones of the mask (folded per wave into one device word, integer atomics only), and the call
 * returns after the stream has finished. */
int pst_polygon_mask_device(const pst_polygon_set* set, const pst_buffer* b, int outside, uint8_t* d_mask, uint64_t* count);
/* The companion of pst_buffer_set_u8_where_device for an overlay: the U8 attribute of that name (interleaved or columnar) =
 * d_values[d_ids[i]] wherever d_ids[i] < n_values; the other points -- 0xFFFFFFFF among them -- keep theirs.  d_ids (len x uint32) and
 * d_values (n_values bytes) in DEVICE memory.  No such U8 attribute -> PST_ERR_MISSING_ATTRIBUTE.  written == NULL: stream-ordered;
 * otherwise *written = the points written, after the stream has finished.  An empty buffer and n_values == 0 are answered on the host. */
int pst_buffer_set_u8_from_ids_device(pst_buffer* b, const char* attribute_name, const uint32_t* d_ids, const uint8_t* d_values, uint32_t n_values, uint64_t* written);
/* The kernels' seams (tests place their sizes around them; each pointer optional): points per workgroup of the flat kernel and of the banded
 * one, and the most entries the flat kernel takes -- also the count up to which the automatic choice takes it.  That count is what the
 * LDS holds: measured at 4, 64, 512 and that many entries, the flat kernel was the faster one every time.  Host only. */
int pst_crop_kernel_shape(uint32_t* flat_points_per_block, uint32_t* banded_points_per_block, uint32_t* flat_max_edges);

/* ---- Segment statistics: per-label count, box, centroid, covariance and value statistics ------------------------------------------------
 * The table of objects behind a segmentation -- lidR's crown_metrics, PCL's compute3DCentroid / computeCovarianceMatrix per cluster,
 * CloudCompare's per-component statistics, PDAL's filters.stats with a `where` (the reference has nothing like it) -- for the labels of
 * pst_euclidean_clusters, pst_dbscan, pst_region_growing, pst_segment_trees_device and pst_points_in_polygons_device, in ONE call for all
 * segments.  Every operation below is a separately rounded f64 operation (no contraction); no square root appears anywhere.
 *   inputs:      d_labels: DEVICE memory, len x u32.  n_segments = S.  v_i = the z of point i (d_values == NULL), or d_values[i]: DEVICE
 *                memory, len x f64.  d_mask: DEVICE memory, len bytes, nullable.
 *   member:      point i is a member of segment s = d_labels[i] iff s < S (0xFFFFFFFF and every label >= S belong to no segment and are
 *                never used as an index), x, y and z are finite, v_i is finite, and d_mask is NULL or d_mask[i] != 0.  The members of s
 *                in ascending buffer index are a_0 .. a_(m-1).
 *   the sum:     every sum below is the fixed tree T (PST_SEGMENT_GROUP = 256 is part of this definition).  A sequence of length L > 1
 *                is cut into consecutive groups of 256; missing elements of the last group are -0.0, the identity of IEEE addition in
 *                round-to-nearest (it changes nothing, zero signs included: a group of one element is that element).  A group gives
 *                r_l = ((g_l + g_(l+64)) + g_(l+128)) + g_(l+192) for l = 0 .. 63, then for h = 32, 16, 8, 4, 2, 1: r_l = r_l + r_(l+h)
 *                for l < h; the group's partial is r_0.  The partials, in order, are the next sequence; repeat until one value is left
 *                (at most 4 levels for any legal length).
 *   statistics:  `stats` is a set of the bits below; 0 or a value above 255 -> PST_ERR_INVALID_ARGUMENT.  out = f64 [planes][S], the
 *                planes of the set bits in ascending bit order.  Per segment with m > 0:
 *                  PST_SEGMENT_COUNT (1)           1 plane   (double)m
 *                  PST_SEGMENT_BOUNDS (2)          6 planes  min x, min y, min z, max x, max y, max z: each a member's bits, -0.0 below +0.0
 *                  PST_SEGMENT_CENTROID (4)        3 planes  c_x = T(x) / (double)m, and y, z alike
 *                  PST_SEGMENT_COVARIANCE (8)      6 planes  xx, xy, xz, yy, yz, zz: with d = p - c per component (the centroid above),
 *                                                            T(d_a * d_b) / (double)m -- the population covariance, in two passes
 *                  PST_SEGMENT_VALUE_MIN (16)      1 plane   the smallest v, -0.0 below +0.0
 *                  PST_SEGMENT_VALUE_MAX (32)      1 plane   the largest v
 *                  PST_SEGMENT_VALUE_MEAN (64)     1 plane   T(v) / (double)m
 *                  PST_SEGMENT_VALUE_VARIANCE (128) 1 plane  T((v - mean) * (v - mean)) / (double)m
 *                A segment without members has COUNT +0.0 and the canonical quiet NaN (0x7FF8000000000000) in every other plane.
 *   apex:        u32 [S], nullable: per segment the lowest buffer index among the members whose v has the bits of VALUE_MAX (the top of
 *                a tree, the ridge point of a roof); 0xFFFFFFFF for a segment without members.
 *   results:     *n_members = the sum of the counts.  out and apex are BOTH in device memory (out_memkind = PST_MEM_DEVICE) or both in
 *                host memory (anything else), the convention of the cluster labels.
 * The result is a function of the points in buffer order, the labels, the values, the mask, S and `stats` alone -- not of the launch shape
 * or the storage kind --, and two calls write the same bytes.  One path: the points are sorted by label with the library's stable radix
 * sort (which is what makes "ascending buffer index" true), x, y, z and v are gathered into sorted columns, and one wave folds every group
 * of 256, level by level; no floating-point atomics and no per-point atomics on per-segment records.
 * Checks, in the order of pst_rasterize: null arguments (b, d_labels, out, n_members) and invalid parameters (stats, n_segments == 0, the
 * memory kind) are answered before a device is looked for; then PST_ERR_MISSING_ATTRIBUTE when Position3D is not stored as Vec3f64; then
 * the device (none: PST_ERR_NO_DEVICE, never a CPU path); then 2^32 - 16 points and more, or n_segments > 2^28 -> PST_ERR_UNSUPPORTED.  An
 * empty buffer is legal: every segment is empty, and out and apex are filled with the empty values (which needs the device).  Out of
 * device memory is PST_ERR_OUT_OF_MEMORY and the next call works.  Synchronous.  Interleaved or columnar, owned, sliced or external, at any
 * byte offset.  Device scratch: 48 bytes per point (16 for the sort's pairs, 32 for the four columns; 40 without d_values) and the sort's
 * own; 28 bytes per segment, 24 more for every further level of the tree, 8 per plane that the second pass needs and `stats` does not
 * name, and the staging of host results; per group of 256 beyond a segment's first, 8 bytes per folded channel. */
enum {
  PST_SEGMENT_COUNT = 1,
  PST_SEGMENT_BOUNDS = 2,
  PST_SEGMENT_CENTROID = 4,
  PST_SEGMENT_COVARIANCE = 8,
  PST_SEGMENT_VALUE_MIN = 16,
  PST_SEGMENT_VALUE_MAX = 32,
  PST_SEGMENT_VALUE_MEAN = 64,
  PST_SEGMENT_VALUE_VARIANCE = 128,
  PST_SEGMENT_GROUP = 256
};
int pst_segment_statistics(const pst_buffer* b, const uint32_t* d_labels, uint32_t n_segments, const double* d_values, const uint8_t* d_mask, uint32_t stats, double* out,
                           uint32_t* apex, uint32_t out_memkind, uint64_t* n_members);
/* The kernels' seams (tests place their sizes around them; each pointer optional; host only): points per workgroup of the key and gather
 * kernels, the group length of the sums (PST_SEGMENT_GROUP), groups per workgroup of the fold kernel (one wave each). */
int pst_segments_kernel_shape(uint32_t* points_per_block, uint32_t* group, uint32_t* groups_per_block);
/* Measurement aid.  With PST_SEGMENTS_TIMES=1 in the environment pst_segment_statistics brackets its three phases with stream events; this
 * returns the calling thread's last call: ms = {keys + sort + directory, gather, folds + output}.  Zeros without the switch.  Host only. */
int pst_segments_phase_times(double ms[3]);

/* ---- Quantiles: per-cell and per-segment order statistics and counts above a threshold ---------------------------------------------------
 * What lidR's zq95 and pzabove2, PDAL's filters.stats percentiles and numpy's quantile per group compute (the reference has nothing like
 * it): the p-quantile of the values of every cell of an XY grid (pst_rasterize_quantiles) or of every segment (pst_segment_quantiles), and
 * the number of values above a threshold, in ONE call for all groups.  Every operation below is a separately rounded f64 operation (no
 * contraction).
 *   groups:      pst_rasterize_quantiles: the cells of pst_rasterize's grid, with that call's grid rules (origin and dim given together or
 *                both NULL: the automatic grid over the finite points, whatever the mask), its inside test and its members: x, y and v_i
 *                finite, d_mask NULL or d_mask[i] != 0, inside.  groups = rows * cols, group = row * cols + col.
 *                pst_segment_quantiles: the segments of pst_segment_statistics with its members: d_labels[i] < S, x, y, z and v_i finite,
 *                d_mask NULL or d_mask[i] != 0.  groups = S.
 *                v_i = the z of point i (d_values == NULL), or d_values[i]: DEVICE memory, len x f64.
 *   order:       s_0 .. s_(m-1) are the values of a group's m members in ascending order of the key that orders the doubles
 *                numerically with -0.0 below +0.0.  Values with equal bits are indistinguishable: there is no tie rule.
 *   quantiles:   probs[0 .. n_probs): HOST doubles in [0, 1]; a NaN or anything outside -> PST_ERR_INVALID_ARGUMENT.  Per p:
 *                  h = (double)(m - 1) * p,  lo = (uint32)floor(h),  g = h - (double)lo
 *                  PST_QUANTILE_LINEAR (0)  s_lo with its bits when g == 0.0, else s_lo + g * (s_(lo+1) - s_lo)   (Hyndman-Fan type 7)
 *                  PST_QUANTILE_LOWER (1)   s_lo
 *                  PST_QUANTILE_HIGHER (2)  s_lo when g == 0.0, else s_(lo+1)
 *                any other `method` -> PST_ERR_INVALID_ARGUMENT.  h <= m - 1 always (the exact product is at most a representable
 *                number, and rounding is monotone); g > 0 means h is no integer, so h < m - 1 and lo + 1 <= m - 1.  p = 0 gives the bits
 *                of the group's MIN, p = 1 the bits of its MAX (pst_rasterize's and pst_segment_statistics' planes).  Beyond this, what
 *                IEEE arithmetic gives is the definition: a difference that overflows gives +-inf or a NaN.
 *   above:       thresholds[0 .. n_thresholds): HOST doubles; a NaN -> PST_ERR_INVALID_ARGUMENT, +-inf is legal.  Per t: (double) the
 *                number of members with v > t, COMPARED AS DOUBLES: -0.0 is not above +0.0, and +0.0 is not above -0.0.
 *   output:      out = f64 [1 + n_probs + n_thresholds][groups]: plane 0 is COUNT = (double)m, then the quantile planes in the order of
 *                probs, then the above planes in the order of thresholds; in device memory (out_memkind = PST_MEM_DEVICE) or host memory
 *                (anything else).  1 <= n_probs + n_thresholds <= 64, else PST_ERR_INVALID_ARGUMENT.  An empty group has COUNT +0.0, the
 *                canonical quiet NaN (0x7FF8000000000000) in every quantile plane and +0.0 in every above plane.
 *   results:     *n_members = the sum of the counts; origin_out, dim_out (each optional) = the grid that was used.
 * The result is a function of the MULTISET of (group, value) pairs and the parameters alone: not of the order of the points in the buffer,
 * the storage kind, the launch shape or the path a group took.  Two calls write the same bytes.  Groups of at most PST_QUANTILES_CAP
 * members are sorted in LDS, many per workgroup, and selected there; larger ones are sorted by two radix sorts (by value, then stably by
 * group).  No floating-point atomics, and no per-point atomics on per-group records.
 * Checks: those of pst_rasterize and of pst_segment_statistics respectively, in their order, with the plane count, the arrays, the
 * probabilities, the method and the thresholds where `stats` is checked there; the same limits (2^32 - 16 points, 2^28 cells or segments),
 * the same empty-buffer rules (automatic grid: PST_OK on the host, nothing written; a given grid or segments: every group empty) and the
 * same out-of-memory behaviour.  Synchronous.  Interleaved or columnar, owned, sliced or external, at any byte offset.  Device scratch: 24
 * bytes per point and the sort's own, 4 per group, the staging of host results, and 44 per member of a group above the cap (DESIGN.md
 * 4.25). */
enum {
  PST_QUANTILE_LINEAR = 0,
  PST_QUANTILE_LOWER = 1,
  PST_QUANTILE_HIGHER = 2,
  PST_QUANTILES_CAP = 512
};
int pst_rasterize_quantiles(const pst_buffer* b, const double* d_values, const uint8_t* d_mask, double cell_size, const double origin[2], const uint32_t dim[2],
                            const double* probs, uint32_t n_probs, uint32_t method, const double* thresholds, uint32_t n_thresholds, double* out, uint32_t out_memkind,
                            double origin_out[2], uint32_t dim_out[2], uint64_t* n_members);
int pst_segment_quantiles(const pst_buffer* b, const uint32_t* d_labels, uint32_t n_segments, const double* d_values, const uint8_t* d_mask, const double* probs,
                          uint32_t n_probs, uint32_t method, const double* thresholds, uint32_t n_thresholds, double* out, uint32_t out_memkind, uint64_t* n_members);
/* The kernels' seams (tests place their sizes around them; each pointer optional; host only): the sorted positions whose groups one
 * workgroup of the LDS kernel owns, the largest group it sorts (PST_QUANTILES_CAP), and the window of sorted positions it loads and sorts
 * at once -- points_per_block + cap - 1 <= window, so a workgroup packs up to points_per_block groups. */
int pst_quantiles_kernel_shape(uint32_t* points_per_block, uint32_t* cap, uint32_t* window);
/* Measurement aid.  With PST_QUANTILES_TIMES=1 in the environment both calls bracket their four phases with stream events; this returns
 * the calling thread's last call: ms = {keys + sort + directory, gather, counts + small groups, large groups}.  Zeros without the switch.
 * Host only. */
int pst_quantiles_phase_times(double ms[4]);

/* ---- Fixed-radius neighbour search ----------------------------------------------------------------------------------------------------
 * What PCL's radiusSearch, Open3D's search_radius_vector_3d, scipy's query_ball_point and PDAL's filters.radialdensity compute (the
 * reference has nothing like it): ALL targets within `radius` of every query, as per-query counts (pst_radius_neighbour_counts_device)
 * or as variable-length lists in CSR form (pst_radius_search_device), over a pst_nn_index, for queries from any buffer (the target's own
 * buffer gives the self-search).  Every operation below is a separately rounded f64 operation (no contraction).
 *   query:       q goes through the optional transform12 exactly as in the nearest-neighbour calls: x' = ((r00*x + r01*y) + r02*z) + t0.
 *   neighbour:   a finite target p is a neighbour of q iff d2 = (dx*dx + dy*dy) + dz*dz <= r2, dx = p.x - q'.x (target minus query),
 *                r2 = radius * radius.  The bound is inclusive.  A query whose transformed position is not finite has no neighbours;
 *                targets that are not finite are never neighbours.  A query that is itself a target finds itself at distance 0 (DBSCAN's
 *                and scipy's convention; there is no exclusion option).
 *   counts:      counts[i] = the number of neighbours of query i, u32.
 *   lists:       offsets = u64 [n + 1], the exclusive sum of the counts; total = offsets[n].  The list of query i is
 *                indices[offsets[i] .. offsets[i + 1]): target BUFFER indices, u32, ordered by ascending (d2, buffer index);
 *                distances[j] = sqrt(d2), correctly rounded, in the same order.
 * The result is a function of the two clouds, the transform and the radius alone: not of the index's cell edge, the launch shape, the
 * storage kind or the path a list took.  Two calls write the same bytes.  No floating-point atomics.
 * pst_radius_neighbour_counts_device: d_counts (DEVICE, n x u32) and total (HOST) are each optional, not both NULL.
 * pst_radius_search_device: d_offsets (DEVICE, n + 1 x u64) and total (HOST) are required; d_indices (DEVICE, capacity x u32), d_distances
 *   (DEVICE, capacity x f64, optional).  d_indices == NULL with capacity == 0 is the COUNTING FORM: offsets and *total are written, nothing is
 *   filled.  total > capacity -> PST_ERR_RANGE with d_offsets and *total written and not one byte of d_indices or d_distances touched (the
 *   pst_plane_inliers convention: size the arrays from *total and call again).  total >= 2^32 - 16 -> PST_ERR_UNSUPPORTED after the count, with
 *   offsets and total written.
 * Checks, in the order of the nearest-neighbour calls: before a device is looked for, NULL arguments, a radius that is not finite or
 * not > 0 or whose square is not a normal number (pst_dbscan's check on eps), a transform entry that is not finite ->
 * PST_ERR_INVALID_ARGUMENT; a query without Position3D stored as Vec3f64 -> PST_ERR_MISSING_ATTRIBUTE; then the device; then the limit of
 * 2^32 - 16 query points.  An empty query writes offsets[0] = 0 and total 0.  An index without a finite target gives all-zero counts.
 * Out of device memory -> PST_ERR_OUT_OF_MEMORY, and the next call works.  Both calls are synchronous.  Interleaved or columnar, owned,
 * sliced or external, at any byte offset.  Lists of at most PST_RADIUS_SORT_CAP entries are ordered in LDS, many per workgroup; longer
 * ones by three stable radix sorts (index, d2, list).
 * Device scratch: per query 28 bytes and the pair sort's own (keys and order of the cell-ordered queries, the counts), 8 more in the
 * counts call (the offsets); per entry 8 bytes (the d2 keys), allocated once the total is known; per entry of a list above the cap 48
 * bytes and the sorts' own, and 16 per such list, allocated once their number is known. */
enum { PST_RADIUS_SORT_CAP = 512 };
int pst_radius_neighbour_counts_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double radius, uint32_t* d_counts, uint64_t* total);
int pst_radius_search_device(const pst_nn_index* index, const pst_buffer* query, const double* transform12, double radius, uint64_t* d_offsets, uint32_t* d_indices,
                             double* d_distances, uint64_t capacity, uint64_t* total);
/* The kernels' seams (tests place their sizes around them; each pointer optional; host only): the queries one workgroup of the count and
 * fill kernels owns, the longest list the LDS kernel orders (PST_RADIUS_SORT_CAP), the window of entries it loads and sorts at once, and
 * the entry positions whose lists it owns -- sort_positions_per_block + sort_cap - 1 <= sort_window. */
int pst_radius_kernel_shape(uint32_t* queries_per_block, uint32_t* sort_cap, uint32_t* sort_window, uint32_t* sort_positions_per_block);
/* Measurement aid.  With PST_RADIUS_TIMES=1 in the environment both calls bracket their phases with stream events; this returns the
 * calling thread's last call: ms = {query keys + sort, count + scan, fill, order}.  Zeros without the switch.  Host only. */
int pst_radius_phase_times(double ms[4]);

/* ---- LAS record encoder (the writer side of the hot path) ---------------------------- */
/* RawLASWriter::write_points_default_layout, pasture-io/src/las/raw_writers.rs:203-363 (+ write_helpers.rs:10-55):
 * `src` holds points in the DEFAULT typed layout of `point_format` (LasPointFormatN::layout(), las_types.rs; interleaved or
 * columnar), `dst` is an interleaved buffer in the exact-binary record layout (las_layout.rs:70-107); records are written
 * to dst[dst_first .. dst_first + len(src)).  X,Y,Z = (((p - offset) / scale) as i64) checked into i32 — a position outside
 * the i32 range is PST_ERR_RANGE ("Position is out of bounds given the current LAS offset and scale!"), like the expect().
 * Header side effects: bounds_inout = {min xyz, max xyz} of the header, updated with strict compares (:28-48; the writer
 * starts from f64::MAX / f64::MIN); points_by_return[r-1] += number of points whose return number is r, 1 <= r <= max_return
 * (5 for legacy headers, 15 with the large_file block, :220-229). */
int pst_las_encode_points(const pst_buffer* src, uint32_t point_format, const double scale[3], const double offset[3], pst_buffer* dst,
                          size_t dst_first, double bounds_inout[6], uint64_t points_by_return[15], uint32_t max_return);
/* Asynchronous, ranged variant for pipelined writers (device-side encode of chunk i overlapping the D2H copy of chunk i-1):
 * encodes source points [src_first, src_first + count) into dst[dst_first ..) on the current stream.  THIS call's header
 * contribution is left in device memory: device_bounds6 = {min xyz, max xyz} seeded with the identities; device_counts16[0] =
 * number of positions outside the i32 range (> 0 is the panic of write_helpers.rs:15-17 — the caller checks it after
 * synchronising), device_counts16[r] = points with return number r (1..max_return). */
int pst_las_encode_range_async(const pst_buffer* src, size_t src_first, size_t count, uint32_t point_format, const double scale[3],
                               const double offset[3], pst_buffer* dst, size_t dst_first, double* device_bounds6, uint64_t* device_counts16,
                               uint32_t max_return);

/* ---- multi-GPU: points shard by index range, the ONLY exchange is the global AABB ------------------------------
 * The reference has no distributed code: its own index-range processing (convert_into_range buffer_conversion.rs:292; 1 MiB chunks
 * raw_readers.rs:309-349) is what shards without a data-path collective, and the seeds of calculate_bounds (bounds.rs:31-32,
 * +f64::MAX / f64::MIN) are the identities an EMPTY shard contributes.  One process per GPU: rank 0 calls pst_comm_unique_id, ships
 * the 128 bytes to the other ranks (any channel), every rank calls pst_comm_init_rank with its device selected (pst_set_device).
 * pst_comm_init is the single-process form (one handle driving GPUs 0..n-1, ncclCommInitAll).  RCCL is bound at run time; without
 * it these entry points return PST_ERR_UNSUPPORTED. */
int pst_comm_unique_id(pst_comm_id* out_id);
int pst_comm_init_rank(int n_ranks, int rank, const pst_comm_id* id, pst_comm** out);
int pst_comm_init(int n_gpus, pst_comm** out);
int pst_comm_size(const pst_comm* comm, int* out_n_ranks);
int pst_comm_destroy(pst_comm* comm);
/* global AABB, in place, stream-ordered (no host synchronisation): device_rec6 = {min xyz, max xyz} as written by
 * pst_calculate_bounds_async / pst_converter_convert_into_range_with_bounds_async.  ONE ncclAllReduce of 6 x f64 with ncclMin over
 * {min xyz, -max xyz} (48 bytes over xGMI: latency-bound).  All-empty input leaves the seeds, i.e. None (bounds.rs:12-14). */
int pst_bounds_allreduce(pst_comm* comm, double* device_rec6);
/* the same for a pst_comm_init handle: device_recs[d] lives on GPU d, streams[d] (array nullable = default streams) is its stream */
int pst_bounds_allreduce_multi(pst_comm* comm, double* const* device_recs, void* const* streams);
/* The sharded path's per-step exchange as ONE launch (round 6): form = 1 registers a device record address -- from then on every AABB record the
 * library is asked to leave THERE (pst_calculate_bounds_async, pst_converter_convert_into_range_with_bounds_async) is written as
 * {min xyz, -max xyz} by the producing kernel's own last fold, pst_bounds_allreduce[_multi] on it is the ncclAllReduce alone (no negation kernels
 * before and after) and the record STAYS in that form: its reader negates components 3..5.  An empty shard's record is +f64::MAX six times
 * (the identities of bounds.rs:31-32).  form = 0 forgets the address.  Unregistered records keep {min, max} and the three-launch exchange. */
int pst_bounds_record_set_form(double* device_rec6, int form);

#ifdef __cplusplus
}
#endif
#endif /* PASTURE_AMD_H */
