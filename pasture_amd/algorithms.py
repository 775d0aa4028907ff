"""pasture-algorithms loops — Python mirror over the C ABI.

  calculate_bounds   pasture-algorithms/src/bounds.rs:11-85
  minmax_attribute   pasture-algorithms/src/minmax.rs:13-51
  transform_attribute  pasture-core/src/containers/point_buffer.rs:391-404 (closed-set transformations)
  compute_normals    pasture-algorithms/src/normal_estimation.rs:79-130
  compute_centroid   pasture-algorithms/src/normal_estimation.rs:198-237
  ransac_plane / ransac_line  pasture-algorithms/src/segmentation.rs:117-370
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .buffers import _Buffer
from .conversion import Transform
from .layout import PointAttributeDefinition


@dataclass(frozen=True)
class AABB:
    """math::AABB<f64>, pasture-core/src/math/bounds.rs:9-26."""
    _min: Tuple[float, float, float]
    _max: Tuple[float, float, float]

    def min(self):
        return self._min

    def max(self):
        return self._max

    def extent(self):
        return tuple(b - a for a, b in zip(self._min, self._max))

    @staticmethod
    def union(a: "AABB", b: "AABB") -> "AABB":  # bounds.rs:109-122
        return AABB(tuple(x if x < y else y for x, y in zip(a._min, b._min)), tuple(x if x > y else y for x, y in zip(a._max, b._max)))


def _phase_times(api, entry: str, phases: int):
    """the `phases` milliseconds behind pst_<entry>: what every *_phase_times below returns"""
    from ._capi import product_api
    ms = (C.c_double * phases)()
    getattr(api or product_api(), entry)(ms)
    return tuple(ms)


def calculate_bounds(buffer: _Buffer) -> Optional[AABB]:
    mn, mx, has = (C.c_double * 3)(), (C.c_double * 3)(), C.c_int()
    buffer.api.calculate_bounds(buffer._h, mn, mx, C.byref(has))
    return AABB(tuple(mn), tuple(mx)) if has.value else None


def calculate_bounds_async(buffer: _Buffer, device_out6_ptr: int) -> None:
    """Stream-ordered: writes {min xyz, max xyz} (seeds +/-f64::MAX) to device memory, no host synchronisation."""
    buffer.api.calculate_bounds_async(buffer._h, C.c_void_p(device_out6_ptr))


def minmax_attribute(buffer: _Buffer, attribute: PointAttributeDefinition):
    """Returns (min, max) as numpy scalars / length-3 arrays of the attribute's datatype, or None for an empty buffer."""
    dt = attribute.datatype()
    nc = dt.num_components()
    mn = np.zeros(nc, dtype=dt.numpy_dtype())
    mx = np.zeros(nc, dtype=dt.numpy_dtype())
    has = C.c_int()
    cdt = dt.to_c()
    buffer.api.minmax_attribute(buffer._h, attribute.name().encode(), C.byref(cdt), mn.ctypes.data_as(C.c_void_p),
                                mx.ctypes.data_as(C.c_void_p), C.byref(has))
    if not has.value:
        return None
    return (mn[0], mx[0]) if nc == 1 else (mn, mx)


def transform_attribute(buffer: _Buffer, attribute: PointAttributeDefinition, transform: Transform) -> None:
    cdt = attribute.datatype().to_c()
    x = transform.to_c()
    buffer.api.transform_attribute(buffer._h, attribute.name().encode(), C.byref(cdt), C.byref(x))


def transform_attribute_expr(buffer: _Buffer, attribute: PointAttributeDefinition, expression: str, device_params=()) -> None:
    """transform_attribute(attribute, |index, value| expression), point_buffer.rs:391-404: a device expression over v, x y z, c, i (the
    closure's index) and p0 .. p3 = `device_params` (addresses of device arrays of double: what the closure would capture)."""
    cdt = attribute.datatype().to_c()
    arr = (C.c_void_p * max(1, len(device_params)))(*[C.c_void_p(int(p)) for p in device_params])
    buffer.api.transform_attribute_expr(buffer._h, attribute.name().encode(), C.byref(cdt), expression.encode(), C.cast(arr, C.POINTER(C.c_void_p)) if device_params else None,
                                        len(device_params))


def compute_normals(point_cloud: _Buffer, k_nn: int, return_knn: bool = False):
    """Vec<(Vector3<f64>, f64)> as (normals (n,3) f64, curvature (n,) f64[, knn indices (n,k) int64])."""
    n = point_cloud.len()
    normals = np.zeros((n, 3), dtype=np.float64)
    curv = np.zeros(n, dtype=np.float64)
    knn = np.full((n, max(k_nn, 1)), -1, dtype=np.int64) if return_knn else None
    point_cloud.api.compute_normals(point_cloud._h, k_nn, normals.ctypes.data_as(C.POINTER(C.c_double)),
                                    curv.ctypes.data_as(C.POINTER(C.c_double)),
                                    knn.ctypes.data_as(C.POINTER(C.c_int64)) if knn is not None else None)
    return (normals, curv, knn) if return_knn else (normals, curv)


def compute_centroid(point_cloud: _Buffer) -> Tuple[float, float, float]:
    """normal_estimation.rs:198-237: mean Position3D (Vec3f64) over all points, over the finite ones when some coordinate is NaN;
    panics (status 11) on an empty cloud."""
    c = (C.c_double * 3)()
    point_cloud.api.compute_centroid(point_cloud._h, c)
    return tuple(c)


def compute_normals_into(point_cloud: _Buffer, k_nn: int, target: _Buffer) -> None:
    """Device-resident: writes NORMAL (Vec3f32) and "Curvature" (F64) attributes of `target`."""
    point_cloud.api.compute_normals_into(point_cloud._h, k_nn, target._h)


def compute_normals_device(point_cloud: _Buffer, k_nn: int, normals_ptr: int = 0, curvature_ptr: int = 0, knn_ptr: int = 0) -> None:
    """The result of compute_normals in caller-owned DEVICE memory (addresses; 0 = not wanted): normals f64 [n][3], curvature f64 [n],
    neighbour lists uint32 [n][k] in ascending distance."""
    point_cloud.api.compute_normals_device(point_cloud._h, k_nn, C.c_void_p(normals_ptr or None), C.c_void_p(curvature_ptr or None),
                                           C.c_void_p(knn_ptr or None))


def reload_tuning(api=None) -> None:
    """The PST_KNN_* switches are read from the environment once per process; this reads them again (tests and A/B harnesses that change
    them inside one process).  The oracle has no such switches: a no-op there."""
    from ._capi import product_api
    api = api or product_api()
    if hasattr(api, "reload_tuning"):
        api.reload_tuning()


def release_scratch(api=None) -> None:
    """Frees the device scratch the calling thread's compute_normals* calls keep between calls (about 55 bytes per point of the largest
    recent cloud, never more than PST_SCRATCH_MAX_BYTES = 16 GiB by default).  Never needed for correctness."""
    from ._capi import product_api
    (api or product_api()).release_scratch()


def voxelgrid_filter(buffer: _Buffer, leafsize_x: float, leafsize_y: float, leafsize_z: float, filtered_buffer: _Buffer) -> None:
    """voxel_grid.rs:109-166: down-samples `buffer` to one centroid per occupied voxel (cells centred on the axis markers),
    appended to `filtered_buffer` in (x, y, z) voxel order; per-attribute reductions of set_all_attributes (:459-689)."""
    buffer.api.voxelgrid_filter(buffer._h, leafsize_x, leafsize_y, leafsize_z, filtered_buffer._h)


class VoxelGridPlan:
    """Stream-ordered voxelgrid_filter (pst_voxelgrid_plan_create / pst_voxelgrid_filter_async): ONE synchronous pass over `buffer` sizes every
    scratch buffer; `filter_async` then runs bounds -> markers -> keys -> sort -> run heads -> reductions on the current stream without a
    host round trip or an allocation (hipGraph-capturable).  `filtered_buffer` must already hold dst_first + max_voxels points; the voxel
    count and a status word (0 = ok) land in the two uint64 at `count_and_status_ptr` (device-accessible memory) in stream order."""

    def __init__(self, buffer: _Buffer, leafsize_x: float, leafsize_y: float, leafsize_z: float):
        self.api = buffer.api
        h, mv = C.c_void_p(), C.c_size_t()
        self.api.voxelgrid_plan_create(buffer._h, leafsize_x, leafsize_y, leafsize_z, C.byref(h), C.byref(mv))
        self._h, self.max_voxels = h, mv.value

    def filter_async(self, buffer: _Buffer, filtered_buffer: _Buffer, dst_first: int, count_and_status_ptr: int) -> None:
        self.api.voxelgrid_filter_async(self._h, buffer._h, filtered_buffer._h, dst_first, C.c_void_p(int(count_and_status_ptr)))

    def destroy(self) -> None:
        if self._h is not None and self._h.value:
            self.api.voxelgrid_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class NormalsPlan:
    """Stream-ordered compute_normals_into (pst_compute_normals_plan_create / pst_compute_normals_into_async): the constructor runs the
    synchronous call once (`target` holds its result) and keeps its decisions; `compute_into_async` replays the pipeline on the current stream
    without a host round trip or an allocation.  Two uint64 at `status_ptr` (device-accessible): [0] = 0 when the result is complete."""

    def __init__(self, point_cloud: _Buffer, k_nn: int, target: _Buffer):
        self.api = point_cloud.api
        h = C.c_void_p()
        self.api.compute_normals_plan_create(point_cloud._h, k_nn, target._h, C.byref(h))
        self._h = h

    def compute_into_async(self, point_cloud: _Buffer, target: _Buffer, status_ptr: int) -> None:
        self.api.compute_normals_into_async(self._h, point_cloud._h, target._h, C.c_void_p(int(status_ptr)))

    def destroy(self) -> None:
        if self._h is not None and self._h.value:
            self.api.normals_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---- RANSAC plane / line segmentation, pasture-algorithms/src/segmentation.rs ------------------------------------------------------------

@dataclass(frozen=True)
class Plane:
    """segmentation.rs:19-28: ax + by + cz + d = 0 (not normalised); ranking = number of inliers."""
    a: float
    b: float
    c: float
    d: float
    ranking: int

    def coefficients(self) -> Tuple[float, float, float, float]:
        return (self.a, self.b, self.c, self.d)


@dataclass(frozen=True)
class Line:
    """segmentation.rs:10-17: the line through `first` and `second`; ranking = number of inliers."""
    first: Tuple[float, float, float]
    second: Tuple[float, float, float]
    ranking: int

    def coefficients(self) -> Tuple[float, ...]:
        return tuple(self.first) + tuple(self.second)


_U64P = C.POINTER(C.c_uint64)


def _u64(a: np.ndarray):
    return a.ctypes.data_as(_U64P)


def ransac_sample_indices(seed: int, n_points: int, iterations: int, per_hypothesis: int, api=None) -> np.ndarray:
    """The seeded sampler (host only): (iterations, per_hypothesis) point indices, per_hypothesis = 3 for planes, 2 for lines; the recipe is in
    include/pasture_amd.h (pst_ransac_sample_indices)."""
    from ._capi import product_api
    out = np.zeros((iterations, per_hypothesis), dtype=np.uint64)
    (api or product_api()).ransac_sample_indices(seed & 0xFFFFFFFFFFFFFFFF, n_points, iterations, per_hypothesis, _u64(out))
    return out


def _ransac_fit(buffer: _Buffer, line: bool, distance_threshold: float, samples, return_rankings: bool):
    per = 2 if line else 3
    samples = np.ascontiguousarray(np.asarray(samples, dtype=np.uint64))
    if samples.ndim != 2 or samples.shape[1] != per:
        raise ValueError(f"samples must have shape (iterations, {per})")
    iterations = samples.shape[0]
    model = (C.c_double * 6)()
    ranking, best = C.c_uint64(), C.c_size_t()
    rankings = np.zeros(iterations, dtype=np.uint64) if return_rankings else None
    fn = buffer.api.ransac_line_fit if line else buffer.api.ransac_plane_fit
    fn(buffer._h, distance_threshold, _u64(samples), iterations, model, C.byref(ranking), C.byref(best), _u64(rankings) if return_rankings else None)
    m = Line(tuple(model[0:3]), tuple(model[3:6]), ranking.value) if line else Plane(model[0], model[1], model[2], model[3], ranking.value)
    return m, best.value, rankings


def ransac_plane_fit(buffer: _Buffer, distance_threshold: float, samples, return_rankings: bool = False):
    """Scores the plane hypotheses through the point triples `samples` (iterations, 3): (Plane, winning iteration[, rankings of all])."""
    m, best, rk = _ransac_fit(buffer, False, distance_threshold, samples, return_rankings)
    return (m, best, rk) if return_rankings else (m, best)


def ransac_line_fit(buffer: _Buffer, distance_threshold: float, samples, return_rankings: bool = False):
    m, best, rk = _ransac_fit(buffer, True, distance_threshold, samples, return_rankings)
    return (m, best, rk) if return_rankings else (m, best)


def _model_array(model, line: bool):
    v = model.coefficients() if isinstance(model, (Plane, Line)) else tuple(model)
    if len(v) != (6 if line else 4):
        raise ValueError("a plane has 4 coefficients, a line 6")
    return (C.c_double * 6)(*v)


def _inliers(buffer: _Buffer, line: bool, model, distance_threshold: float, capacity: Optional[int]) -> np.ndarray:
    fn = buffer.api.line_inliers if line else buffer.api.plane_inliers
    arr = _model_array(model, line)
    count = C.c_uint64()
    if capacity is None:
        fn(buffer._h, arr, distance_threshold, None, 0, C.byref(count))
        capacity = count.value
    out = np.zeros(capacity, dtype=np.uint64)
    fn(buffer._h, arr, distance_threshold, _u64(out), capacity, C.byref(count))
    return out[:count.value]


def plane_inliers(buffer: _Buffer, plane, distance_threshold: float, capacity: Optional[int] = None) -> np.ndarray:
    """Indices (ascending, uint64) of the points closer to `plane` (a Plane or (a, b, c, d)) than distance_threshold."""
    return _inliers(buffer, False, plane, distance_threshold, capacity)


def line_inliers(buffer: _Buffer, line, distance_threshold: float, capacity: Optional[int] = None) -> np.ndarray:
    return _inliers(buffer, True, line, distance_threshold, capacity)


def plane_inlier_mask(buffer: _Buffer, plane, distance_threshold: float, device_mask_ptr: int) -> None:
    """Stream-ordered: writes len(buffer) bytes (1 = inlier) to DEVICE memory at device_mask_ptr -- the mask filter_into / filter_into_async take
    as (device_mask_ptr, 'device')."""
    buffer.api.plane_inlier_mask_device(buffer._h, _model_array(plane, False), distance_threshold, C.c_void_p(int(device_mask_ptr)))


def line_inlier_mask(buffer: _Buffer, line, distance_threshold: float, device_mask_ptr: int) -> None:
    buffer.api.line_inlier_mask_device(buffer._h, _model_array(line, True), distance_threshold, C.c_void_p(int(device_mask_ptr)))


def _ransac(buffer: _Buffer, line: bool, distance_threshold: float, num_of_iterations: int, seed: int, samples):
    if samples is None:
        model = (C.c_double * 6)()
        ranking = C.c_uint64()
        fn = buffer.api.ransac_line if line else buffer.api.ransac_plane
        fn(buffer._h, distance_threshold, num_of_iterations, seed & 0xFFFFFFFFFFFFFFFF, model, C.byref(ranking))
        m = Line(tuple(model[0:3]), tuple(model[3:6]), ranking.value) if line else Plane(model[0], model[1], model[2], model[3], ranking.value)
    else:
        samples = np.asarray(samples, dtype=np.uint64)
        if samples.shape[0] != num_of_iterations:
            raise ValueError("samples must hold num_of_iterations hypotheses")
        m = _ransac_fit(buffer, line, distance_threshold, samples, False)[0]
    return m, _inliers(buffer, line, m, distance_threshold, m.ranking)


def ransac_plane(buffer: _Buffer, distance_threshold: float, num_of_iterations: int, seed: int = 0, samples=None):
    """ransac_plane_serial, segmentation.rs:233-256: (Plane, indices of its inliers as uint64, ascending).  The reference's hypotheses come from
    rand::thread_rng(); here from the seeded sampler (ransac_sample_indices) or from `samples` (num_of_iterations, 3)."""
    return _ransac(buffer, False, distance_threshold, num_of_iterations, seed, samples)


def ransac_line(buffer: _Buffer, distance_threshold: float, num_of_iterations: int, seed: int = 0, samples=None):
    """ransac_line_serial, segmentation.rs:341-370: (Line, indices of its inliers)."""
    return _ransac(buffer, True, distance_threshold, num_of_iterations, seed, samples)


def ransac_kernel_shape(api=None) -> dict:
    """The scoring kernel's seams: points per wave, per workgroup, workgroups per compute unit of one grid pass, hypotheses per pass."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(4)]
    (api or product_api()).ransac_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_wave", "points_per_block", "blocks_per_cu", "batch"), (x.value for x in v)))


# ---- kNN search with distances, statistical and radius outlier removal (include/pasture_amd.h) ---------------------------------------------

class _DeviceArray:
    """`count` values of one scalar datatype in device memory the library owns: a one-attribute columnar buffer (no torch needed)."""

    def __init__(self, api, datatype, count: int):
        from .buffers import HashMapBuffer
        from .layout import PointLayout
        self.attribute = PointAttributeDefinition.custom("Values", datatype)
        self.buffer = HashMapBuffer.new_from_layout(PointLayout.from_attributes([self.attribute], api=api))
        self.buffer.resize(count)
        self.ptr = self.buffer.column_ptr(self.attribute)

    def to_numpy(self) -> np.ndarray:
        return self.buffer.view_attribute(self.attribute)


def knn_search_device(point_cloud: _Buffer, k: int, distances_ptr: int, knn_ptr: int = 0) -> None:
    """The neighbour lists of compute_normals with their distances, in caller-owned DEVICE memory: distances f64 [n][k] (required), indices
    uint32 [n][k] (0 = not wanted), both in ascending distance; a padded slot is 0xFFFFFFFF at distance +inf."""
    point_cloud.api.knn_search_device(point_cloud._h, k, C.c_void_p(knn_ptr or None), C.c_void_p(distances_ptr or None))


def knn_search(point_cloud: _Buffer, k: int):
    """(indices (n, k) int64 with -1 padding, distances (n, k) float64): the k nearest neighbours of every point, itself included, ascending."""
    from .layout import PointAttributeDataType as T
    n = point_cloud.len()
    count = n * max(k, 0) if 3 <= k <= 64 and n >= 3 else 0  # (anything else is answered by the call's own checks)
    knn, dist = _DeviceArray(point_cloud.api, T.U32, count), _DeviceArray(point_cloud.api, T.F64, count)
    point_cloud.api.knn_search_device(point_cloud._h, k, C.c_void_p(knn.ptr or None), C.c_void_p(dist.ptr or 1))
    idx = knn.to_numpy().astype(np.int64).reshape(n, k)
    idx[idx == 0xFFFFFFFF] = -1
    return idx, dist.to_numpy().reshape(n, k)


@dataclass(frozen=True)
class OutlierStatistics:
    """What the statistical criterion measured: over the `count` points with a finite mean neighbour distance, its mean and (sample) standard
    deviation; threshold = mean + stddev_mult * stddev; kept = points with a finite mean distance <= threshold."""
    mean: float
    stddev: float
    threshold: float
    count: int
    kept: int


def statistical_outlier_mask(buffer: _Buffer, mean_k: int, stddev_mult: float, device_mask_ptr: Optional[int] = None, return_mean_distances: bool = False):
    """PCL's / PDAL's statistical outlier criterion on the device: per point the mean distance to its mean_k nearest neighbours; keep those
    within mean + stddev_mult * stddev of all points' means.  Returns (mask, OutlierStatistics[, mean distances (n,) float64]); mask is a
    numpy uint8 array (1 = keep), or None when the bytes went to DEVICE memory at device_mask_ptr -- what filter takes as (ptr, 'device')."""
    from .layout import PointAttributeDataType as T
    n = buffer.len()
    stats, kept = (C.c_double * 4)(), C.c_uint64()
    mask = np.zeros(n, dtype=np.uint8) if device_mask_ptr is None else None
    dbar = _DeviceArray(buffer.api, T.F64, n if 1 <= mean_k <= 63 and n >= max(3, mean_k + 1) else 0) if return_mean_distances else None
    ptr = C.c_void_p(int(device_mask_ptr) or None) if mask is None else C.c_void_p(mask.ctypes.data if n else 1)
    buffer.api.statistical_outlier_mask(buffer._h, mean_k, stddev_mult, ptr, 0 if mask is None else 1, C.c_void_p(dbar.ptr or None) if dbar else None, stats,
                                        C.byref(kept))
    st = OutlierStatistics(stats[0], stats[1], stats[2], int(stats[3]), kept.value)
    return (mask, st, dbar.to_numpy()) if return_mean_distances else (mask, st)


def radius_outlier_mask(buffer: _Buffer, radius: float, min_neighbours: int, device_mask_ptr: Optional[int] = None):
    """Keep the points with at least min_neighbours other points within `radius`.  Returns (mask, kept); mask as in statistical_outlier_mask."""
    n = buffer.len()
    kept = C.c_uint64()
    mask = np.zeros(n, dtype=np.uint8) if device_mask_ptr is None else None
    ptr = C.c_void_p(int(device_mask_ptr) or None) if mask is None else C.c_void_p(mask.ctypes.data if n else 1)
    buffer.api.radius_outlier_mask(buffer._h, radius, min_neighbours, ptr, 0 if mask is None else 1, C.byref(kept))
    return mask, kept.value


def _filter_by_device_mask(buffer: _Buffer, out_buffer_type, fill, whole_array: bool = False):
    """fill(address of the mask's bytes) -- or, with whole_array, fill(the _DeviceArray that holds them) -- writes the mask and returns the call's second result"""
    from .layout import PointAttributeDataType as T
    mask = _DeviceArray(buffer.api, T.U8, buffer.len())
    result = fill(mask if whole_array else mask.ptr)
    return buffer.filter(out_buffer_type or type(buffer), (mask.ptr, "device")), result


def remove_statistical_outliers(buffer: _Buffer, mean_k: int, stddev_mult: float, out_buffer_type=None):
    """(the points statistical_outlier_mask keeps, OutlierStatistics): mask and compaction stay in device memory.  `buffer` is columnar
    (filter is defined on HashMapBuffer)."""
    return _filter_by_device_mask(buffer, out_buffer_type, lambda p: statistical_outlier_mask(buffer, mean_k, stddev_mult, device_mask_ptr=p)[1])


def remove_radius_outliers(buffer: _Buffer, radius: float, min_neighbours: int, out_buffer_type=None):
    """(the points radius_outlier_mask keeps, their number)."""
    return _filter_by_device_mask(buffer, out_buffer_type, lambda p: radius_outlier_mask(buffer, radius, min_neighbours, device_mask_ptr=p)[1])


def outlier_kernel_shape(api=None) -> dict:
    """The seams of the outlier kernels: points per workgroup of the distance kernels, threads of the workgroup that adds the block partials of
    the sums, points per block partial."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).outlier_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "reduce_block", "reduce_points_per_block"), (x.value for x in v)))


# ---- Euclidean cluster extraction (include/pasture_amd.h) ------------------------------------------------------------------------------------

NO_CLUSTER = 0xFFFFFFFF
_MAX_SIZE = 2 ** 64 - 1


def euclidean_clusters(buffer: _Buffer, tolerance: float, min_size: int = 1, max_size: int = _MAX_SIZE, device_labels_ptr: Optional[int] = None):
    """PCL's EuclideanClusterExtraction / PDAL's filters.cluster on the device: connected components of "closer than `tolerance`" over the
    finite points, those of min_size .. max_size points kept and numbered by descending size (ties: ascending smallest member index).
    Returns (labels, sizes): labels is a numpy uint32 array (NO_CLUSTER = 0xFFFFFFFF where a point is in no kept cluster), or None when the
    len(buffer) uint32 values went to DEVICE memory at device_labels_ptr; sizes is a numpy uint64 array, sizes[c] = points of cluster c.
    Two calls: the first writes the labels and reports the number of clusters, the second fetches that many sizes."""
    n = buffer.len()
    labels = np.full(n, NO_CLUSTER, dtype=np.uint32) if device_labels_ptr is None else None
    ptr = C.c_void_p(int(device_labels_ptr) or None) if labels is None else C.c_void_p(labels.ctypes.data if n else 1)
    kind = 0 if labels is None else 1
    count, clustered = C.c_uint64(), C.c_uint64()
    call = buffer.api.euclidean_clusters
    call(buffer._h, tolerance, min_size, max_size, ptr, kind, None, 0, C.byref(count), C.byref(clustered))
    sizes = np.zeros(count.value, dtype=np.uint64)
    if count.value:
        call(buffer._h, tolerance, min_size, max_size, ptr, kind, _u64(sizes), count.value, C.byref(count), C.byref(clustered))
    return labels, sizes


def cluster_mask(device_labels_ptr: int, n: int, first_cluster: int, cluster_count: int, device_mask_ptr: int, api=None) -> None:
    """Stream-ordered: mask[i] = 1 iff first_cluster <= labels[i] < first_cluster + cluster_count, both arrays (n uint32 / n bytes) in DEVICE
    memory -- the mask filter / filter_into take as (device_mask_ptr, 'device').  NO_CLUSTER is never selected."""
    from ._capi import product_api
    (api or product_api()).cluster_mask_device(C.c_void_p(int(device_labels_ptr) or None), n, first_cluster, cluster_count, C.c_void_p(int(device_mask_ptr) or None))


def extract_clusters(buffer: _Buffer, tolerance: float, min_size: int = 1, max_size: int = _MAX_SIZE, first_cluster: int = 0, cluster_count: int = 1,
                     out_buffer_type=None):
    """(the points of clusters first_cluster .. first_cluster + cluster_count - 1 in buffer order with all their attributes, sizes of ALL kept
    clusters): labels and mask stay in device memory.  `buffer` is columnar (filter is defined on HashMapBuffer)."""
    from .layout import PointAttributeDataType as T
    labels = _DeviceArray(buffer.api, T.U32, buffer.len())

    def fill(mask_ptr):
        sizes = euclidean_clusters(buffer, tolerance, min_size, max_size, device_labels_ptr=labels.ptr or 1)[1]
        cluster_mask(labels.ptr, buffer.len(), first_cluster, cluster_count, mask_ptr, api=buffer.api)
        return sizes
    return _filter_by_device_mask(buffer, out_buffer_type, fill)


def cluster_kernel_shape(api=None) -> dict:
    """The seams of the traversal kernel: points one workgroup owns, points of one LDS candidate tile (0: candidates are not staged)."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).cluster_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "tile_points"), (x.value for x in v)))


def cluster_phase_times(api=None):
    """(index build, traversal + union, bookkeeping) in milliseconds of this thread's last euclidean_clusters call; zeros unless
    PST_CLUSTER_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "cluster_phase_times", 3)


# ---- DBSCAN (include/pasture_amd.h) ------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class DbscanResult:
    labels: Optional[np.ndarray]  # uint32, NO_CLUSTER for noise and non-finite points; None when they went to device memory
    core: Optional[np.ndarray]    # bool, True for core points; None when it went to device memory
    sizes: np.ndarray             # uint64, sizes[c] = core + border points of cluster c
    n_core: int
    n_labelled: int


def dbscan(buffer: _Buffer, eps: float, min_points: int, device_labels_ptr: Optional[int] = None, device_core_ptr: Optional[int] = None) -> DbscanResult:
    """PDAL's filters.dbscan / scikit-learn's DBSCAN on the device: a finite point with at least `min_points` points within `eps` (itself
    included) is a core point; clusters are the connected components of the core points; a point that is not core joins the cluster of its
    nearest core neighbour (ties: smallest buffer index) and bridges nothing; the rest is noise.  Clusters are numbered by descending size
    (ties: ascending smallest member index).  With device_labels_ptr the len(buffer) uint32 labels and, at device_core_ptr (optional), the
    len(buffer) core bytes go to DEVICE memory and the result's labels / core are None.
    Two calls: the first writes labels and core flags and reports the number of clusters, the second fetches that many sizes."""
    n = buffer.len()
    on_device = device_labels_ptr is not None
    if device_core_ptr is not None and not on_device:
        raise ValueError("device_core_ptr needs device_labels_ptr: labels and core flags share one memory kind")
    labels = None if on_device else np.full(n, NO_CLUSTER, dtype=np.uint32)
    core = None if on_device else np.zeros(n, dtype=np.uint8)
    if on_device:
        lptr, cptr = C.c_void_p(int(device_labels_ptr) or None), C.c_void_p(int(device_core_ptr) if device_core_ptr else None)
    else:
        lptr, cptr = C.c_void_p(labels.ctypes.data if n else 1), C.c_void_p(core.ctypes.data if n else 1)
    kind = 0 if on_device else 1
    counts = (C.c_uint64 * 3)()
    call = buffer.api.dbscan
    call(buffer._h, eps, min_points, lptr, cptr, kind, None, 0, counts)
    sizes = np.zeros(counts[0], dtype=np.uint64)
    if counts[0]:
        call(buffer._h, eps, min_points, lptr, cptr, kind, _u64(sizes), counts[0], counts)
    return DbscanResult(labels, None if core is None else core.astype(bool), sizes, int(counts[1]), int(counts[2]))


def extract_dbscan_clusters(buffer: _Buffer, eps: float, min_points: int, first_cluster: int = 0, cluster_count: int = 1, out_buffer_type=None):
    """(the points of DBSCAN clusters first_cluster .. first_cluster + cluster_count - 1 in buffer order with all their attributes, sizes of
    ALL clusters): labels and mask stay in device memory.  cluster_count = 0xFFFFFFFF from cluster 0 drops the noise and keeps the rest.
    `buffer` is columnar (filter is defined on HashMapBuffer)."""
    from .layout import PointAttributeDataType as T
    labels = _DeviceArray(buffer.api, T.U32, buffer.len())

    def fill(mask_ptr):
        sizes = dbscan(buffer, eps, min_points, device_labels_ptr=labels.ptr or 1).sizes
        cluster_mask(labels.ptr, buffer.len(), first_cluster, cluster_count, mask_ptr, api=buffer.api)
        return sizes
    return _filter_by_device_mask(buffer, out_buffer_type, fill)


def dbscan_kernel_shape(api=None) -> dict:
    """The seam of the count, link and border kernels: points one workgroup owns, one lane each."""
    from ._capi import product_api
    v = C.c_uint32()
    (api or product_api()).dbscan_kernel_shape(C.byref(v))
    return {"points_per_block": v.value}


def dbscan_phase_times(api=None):
    """(index build, core count, link, border + bookkeeping) in milliseconds of this thread's last dbscan call; zeros unless
    PST_DBSCAN_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "dbscan_phase_times", 4)


# ---- region growing: smooth surface patches (include/pasture_amd.h) --------------------------------------------------------------------------

@dataclass(frozen=True)
class RegionGrowingResult:
    labels: Optional[np.ndarray]  # uint32, NO_CLUSTER for points in no kept region; None when they went to device memory
    smooth: Optional[np.ndarray]  # bool, True for smooth points; None when it went to device memory or was not asked for
    sizes: np.ndarray             # uint64, sizes[c] = smooth + rim points of region c
    n_smooth: int
    n_labelled: int
    normals: Optional[np.ndarray] = None    # (n, 3) float64, region_growing(return_inputs=True): what the regions were grown from
    curvature: Optional[np.ndarray] = None  # (n,) float64
    knn: Optional[np.ndarray] = None        # (n, k) uint32, 0xFFFFFFFF padding

_REGION_SIZES_FIRST = 1 << 16  # sizes asked for by the first call; more regions than that cost a second one


def _region_call(buffer: _Buffer, call, device_labels_ptr, device_smooth_ptr, want_smooth: bool):
    """call(labels, smooth, memkind, sizes, capacity, counts) runs one of the two entries; (labels, smooth, sizes, counts) with the sizes complete"""
    n = buffer.len()
    on_device = device_labels_ptr is not None
    if device_smooth_ptr is not None and not on_device:
        raise ValueError("device_smooth_ptr needs device_labels_ptr: labels and smooth mask share one memory kind")
    labels = None if on_device else np.full(n, NO_CLUSTER, dtype=np.uint32)
    smooth = None if on_device or not want_smooth else np.zeros(n, dtype=np.uint8)
    if on_device:
        lptr, sptr = C.c_void_p(int(device_labels_ptr) or None), C.c_void_p(int(device_smooth_ptr) if device_smooth_ptr else None)
    else:
        lptr, sptr = C.c_void_p(labels.ctypes.data if n else 1), C.c_void_p((smooth.ctypes.data if n else 1) if smooth is not None else None)
    kind = 0 if on_device else 1
    counts = (C.c_uint64 * 3)()
    sizes = np.zeros(min(n, _REGION_SIZES_FIRST), dtype=np.uint64)
    from ._capi import ERR_RANGE, PastureError
    try:
        call(lptr, sptr, kind, _u64(sizes), len(sizes), counts)
    except PastureError as e:
        if e.code != ERR_RANGE:
            raise
        sizes = np.zeros(counts[0], dtype=np.uint64)  # (the counts are set and the labels written: only the sizes are missing)
        call(lptr, sptr, kind, _u64(sizes), len(sizes), counts)
    return labels, None if smooth is None else smooth.astype(bool), sizes[:counts[0]].copy(), counts


def _device_input(api, values, datatype, dtype, count: int, what: str):
    """(address, keep-alive) of `count` values: a caller's device address as it is, a numpy array copied into a device array of the library's"""
    if values is None:
        return 0, None
    if isinstance(values, (int, np.integer)):
        return int(values), None
    a = np.ascontiguousarray(values)
    if a.size != count:
        raise ValueError(f"{what} must hold {count} values")
    if dtype == np.uint32:
        if a.dtype.kind not in "iu":
            raise ValueError(f"{what} must be an integer array")
        a = (a.astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32)  # (-1: no neighbour)
    else:
        a = a.astype(dtype).reshape(-1)
    dev = _DeviceArray(api, datatype, count)
    if count:
        dev.buffer.set_attribute_range(dev.attribute, range(0, count), a)
    return dev.ptr or 1, dev


def region_growing_from_knn(buffer: _Buffer, k: int, knn, normals, curvature=None, min_abs_cos: float = 1.0, curvature_threshold: float = float("inf"),
                            max_distance: float = float("inf"), min_size: int = 1, max_size: int = _MAX_SIZE, device_labels_ptr: Optional[int] = None,
                            device_smooth_ptr: Optional[int] = None, return_smooth: bool = True) -> RegionGrowingResult:
    """Smooth surface patches over given neighbour lists: knn (n, k) integers (-1 or anything >= n: no neighbour), normals (n, 3) and an
    optional curvature (n,), each a numpy array or the address of such an array in DEVICE memory (uint32 / float64).  A point is smooth when
    its normal is finite and its curvature <= curvature_threshold; smooth points whose normals agree, |ni . nj| >= min_abs_cos, and of which
    one lists the other (within max_distance) are in one region; a point that is not smooth joins the region of its first agreeing smooth
    neighbour and bridges nothing.  Regions of min_size .. max_size points are kept and numbered by descending size (ties: ascending smallest
    member index).  With device_labels_ptr the labels and, at device_smooth_ptr (optional), the smooth bytes go to DEVICE memory."""
    from .layout import PointAttributeDataType as T
    n = buffer.len()
    k = int(k)
    count = n * k if 1 <= k <= 64 else 0
    kp, keep_k = _device_input(buffer.api, knn, T.U32, np.uint32, count, "knn")
    np_, keep_n = _device_input(buffer.api, normals, T.F64, np.float64, n * 3, "normals")
    cp, keep_c = _device_input(buffer.api, curvature, T.F64, np.float64, n, "curvature")

    def call(lptr, sptr, kind, sizes, capacity, counts):
        buffer.api.region_growing_from_knn(buffer._h, k, C.c_void_p(kp or None), C.c_void_p(np_ or None), C.c_void_p(cp or None), min_abs_cos, curvature_threshold,
                                           max_distance, min_size, max_size, lptr, sptr, kind, sizes, capacity, counts)
    labels, smooth, sizes, counts = _region_call(buffer, call, device_labels_ptr, device_smooth_ptr, return_smooth)
    del keep_k, keep_n, keep_c
    return RegionGrowingResult(labels, smooth, sizes, int(counts[1]), int(counts[2]))


def region_growing(buffer: _Buffer, k: int, smoothness_deg: float = 10.0, curvature_threshold: float = 0.02, max_distance: float = float("inf"), min_size: int = 1,
                   max_size: int = _MAX_SIZE, min_abs_cos: Optional[float] = None, device_labels_ptr: Optional[int] = None, device_smooth_ptr: Optional[int] = None,
                   return_smooth: bool = True, return_inputs: bool = False, normals_ptr: int = 0, curvature_ptr: int = 0, knn_ptr: int = 0) -> RegionGrowingResult:
    """PCL's RegionGrowing on the device, in its order-free form: the library searches the k nearest neighbours (k = 3 .. 64), takes the normal
    and the curvature (surface variation l3 / (l1 + l2 + l3)) of every point from their covariance, and grows regions as
    region_growing_from_knn does.  Normals agree when the angle between them is at most smoothness_deg degrees (either orientation); the C
    ABI takes min_abs_cos = cos of that angle, which can be given directly instead.  return_inputs: the result also carries the normals,
    curvature and lists the regions were grown from; normals_ptr / curvature_ptr / knn_ptr: DEVICE memory that receives them."""
    import math
    from .layout import PointAttributeDataType as T
    n = buffer.len()
    k = int(k)
    if min_abs_cos is None:
        min_abs_cos = math.cos(math.radians(smoothness_deg))
    kept = {}
    if return_inputs:
        ok = 3 <= k <= 64 and n >= 3  # (anything else is answered by the call's own checks)
        kept = {"normals": _DeviceArray(buffer.api, T.F64, n * 3 if ok else 0), "curvature": _DeviceArray(buffer.api, T.F64, n if ok else 0),
                "knn": _DeviceArray(buffer.api, T.U32, n * k if ok else 0)}
        normals_ptr, curvature_ptr, knn_ptr = kept["normals"].ptr or 0, kept["curvature"].ptr or 0, kept["knn"].ptr or 0

    def call(lptr, sptr, kind, sizes, capacity, counts):
        buffer.api.region_growing(buffer._h, k, min_abs_cos, curvature_threshold, max_distance, min_size, max_size, lptr, sptr, kind, sizes, capacity, counts,
                                  C.c_void_p(int(normals_ptr) or None), C.c_void_p(int(curvature_ptr) or None), C.c_void_p(int(knn_ptr) or None))
    labels, smooth, sizes, counts = _region_call(buffer, call, device_labels_ptr, device_smooth_ptr, return_smooth)
    extra = {}
    if return_inputs:
        extra = {"normals": kept["normals"].to_numpy().reshape(-1, 3), "curvature": kept["curvature"].to_numpy(), "knn": kept["knn"].to_numpy().reshape(-1, max(k, 1))}
    return RegionGrowingResult(labels, smooth, sizes, int(counts[1]), int(counts[2]), **extra)


def extract_regions(buffer: _Buffer, k: int, first_region: int = 0, region_count: int = 1, out_buffer_type=None, **parameters):
    """(the points of regions first_region .. first_region + region_count - 1 in buffer order with all their attributes, sizes of ALL kept
    regions): labels and mask stay in device memory.  region_count = 0xFFFFFFFF from region 0 drops the unlabelled points and keeps the rest.
    parameters: those of region_growing.  `buffer` is columnar (filter is defined on HashMapBuffer)."""
    from .layout import PointAttributeDataType as T
    labels = _DeviceArray(buffer.api, T.U32, buffer.len())

    def fill(mask_ptr):
        sizes = region_growing(buffer, k, device_labels_ptr=labels.ptr or 1, **parameters).sizes
        cluster_mask(labels.ptr, buffer.len(), first_region, region_count, mask_ptr, api=buffer.api)
        return sizes
    return _filter_by_device_mask(buffer, out_buffer_type, fill)


def region_kernel_shape(k: int, api=None) -> dict:
    """The seams of the link kernel at this k: points whose whole neighbour lists one workgroup owns, and its threads."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).region_kernel_shape(k, *[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "threads"), (x.value for x in v)))


def region_phase_times(api=None):
    """(search + features, classify + link, attach + numbering) in milliseconds of this thread's last region growing call; zeros unless
    PST_REGION_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "region_phase_times", 3)


# ---- ground classification: the progressive morphological filter (include/pasture_amd.h) -------------------------------------------------------

@dataclass(frozen=True)
class PmfParameters:
    """The parameters of PDAL's filters.pmf / PCL's ProgressiveMorphologicalFilter (Zhang et al. 2003), with their usual defaults: the raster's
    cell, the largest window (both in the units of the coordinates), the terrain slope, the height thresholds of the first and of the later
    windows, and the growth of the windows' half-widths in cells: base^k (exponential) or (k + 1) * base."""
    cell_size: float = 1.0
    max_window_size: float = 33.0
    slope: float = 1.0
    initial_distance: float = 0.15
    max_distance: float = 2.5
    exponential: bool = True
    base: int = 2

    def c_args(self):
        """the seven scalars the C entry points take, in their order"""
        return (self.cell_size, self.max_window_size, self.slope, self.initial_distance, self.max_distance, 1 if self.exponential else 0, self.base)


def pmf_schedule(params: PmfParameters = PmfParameters(), api=None):
    """(half-widths in cells as uint32, thresholds as float64) of the windows `params` open the raster with.  Host only."""
    from ._capi import product_api
    h, th, count = np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.float64), C.c_uint32()
    (api or product_api()).pmf_schedule(*params.c_args(), h.ctypes.data_as(C.POINTER(C.c_uint32)), th.ctypes.data_as(C.POINTER(C.c_double)), C.byref(count))
    return h[:count.value].copy(), th[:count.value].copy()


def pmf_grid(buffer: _Buffer, cell_size: float) -> dict:
    """The raster ground_mask would lay over the finite points: origin (x0, y0), cols, rows, and the number of finite points (zeros without one)."""
    origin, dim, finite = (C.c_double * 2)(), (C.c_uint32 * 2)(), C.c_uint64()
    buffer.api.pmf_grid(buffer._h, cell_size, origin, dim, C.byref(finite))
    return {"origin": (origin[0], origin[1]), "cols": dim[0], "rows": dim[1], "n_finite": finite.value}


def ground_mask(buffer: _Buffer, params: PmfParameters = PmfParameters(), device_mask_ptr: Optional[int] = None, return_surfaces: bool = False):
    """The progressive morphological ground filter on the device.  Returns (mask, n_ground[, surfaces]): mask is a numpy uint8 array (1 =
    ground), or None when the len(buffer) bytes went to DEVICE memory at device_mask_ptr -- what filter takes as (ptr, 'device'); surfaces is
    a dict of the three float64 (rows, cols) rasters "min_z" (+inf: empty cell), "opened" (the last opened surface) and "limit" (a point is
    ground iff its z is not above its cell's limit), with the raster's "origin" (x0, y0) and "cell_size"."""
    n = buffer.len()
    mask = np.zeros(n, dtype=np.uint8) if device_mask_ptr is None else None
    ptr = C.c_void_p(int(device_mask_ptr) or None) if mask is None else C.c_void_p(mask.ctypes.data if n else 1)
    count = C.c_uint64()
    surfaces, grid = None, None
    if return_surfaces:
        grid = pmf_grid(buffer, params.cell_size)
        surfaces = np.full((3, grid["rows"], grid["cols"]), np.inf, dtype=np.float64)
    sptr = C.c_void_p(surfaces.ctypes.data) if surfaces is not None and surfaces.size else None
    buffer.api.pmf_ground_mask(buffer._h, *params.c_args(), ptr, 0 if mask is None else 1, sptr, 1, C.byref(count))
    if not return_surfaces:
        return mask, count.value
    return mask, count.value, {"min_z": surfaces[0], "opened": surfaces[1], "limit": surfaces[2], "origin": grid["origin"], "cell_size": params.cell_size}


def finite_mask(buffer: _Buffer, device_mask_ptr: int) -> None:
    """Stream-ordered: len(buffer) bytes in DEVICE memory, 1 where x, y and z of the Position3D are all finite."""
    buffer.api.finite_mask_device(buffer._h, C.c_void_p(int(device_mask_ptr) or None))


def set_u8_where(buffer: _Buffer, attribute: PointAttributeDefinition, device_mask_ptr: int, value: int) -> None:
    """Stream-ordered: the U8 attribute = value wherever the byte of the DEVICE mask is not zero; the other points keep theirs."""
    buffer.api.buffer_set_u8_where_device(buffer._h, attribute.name().encode(), C.c_void_p(int(device_mask_ptr) or None), value)


def classify_ground(buffer: _Buffer, params: PmfParameters = PmfParameters(), ground_class: int = 2, other_class: Optional[int] = None) -> int:
    """Writes the LAS Classification (U8) of `buffer` in place on the device: ground_class (2 in the LAS specification) for the ground points;
    other_class for every other point, or, with None, whatever class they have.  Returns the number of ground points."""
    from .layout import PointAttributeDataType as T, attributes as A
    n = buffer.len()
    if n == 0:  # (the call's own checks of the parameters and the layout, answered on the host)
        set_u8_where(buffer, A.CLASSIFICATION, 0, ground_class)
        return ground_mask(buffer, params)[1]
    mask = _DeviceArray(buffer.api, T.U8, n)
    ground = ground_mask(buffer, params, device_mask_ptr=mask.ptr or 1)[1]
    if other_class is not None and n:  # every point first, through a mask of ones (one byte per point from the host: the library has no fill entry point)
        ones = _DeviceArray(buffer.api, T.U8, n)
        ones.buffer.set_attribute_range(ones.attribute, range(0, n), np.ones(n, dtype=np.uint8))
        set_u8_where(buffer, A.CLASSIFICATION, ones.ptr, other_class)
    set_u8_where(buffer, A.CLASSIFICATION, mask.ptr, ground_class)
    buffer.api.stream_synchronize()  # (the mask is released when this returns)
    return ground


def extract_ground(buffer: _Buffer, params: PmfParameters = PmfParameters(), out_buffer_type=None):
    """(the ground points in buffer order with all their attributes, their number): mask and compaction stay in device memory.  `buffer` is
    columnar (filter is defined on HashMapBuffer)."""
    return _filter_by_device_mask(buffer, out_buffer_type, lambda p: ground_mask(buffer, params, device_mask_ptr=p or 1)[1])


def remove_ground(buffer: _Buffer, params: PmfParameters = PmfParameters(), out_buffer_type=None):
    """(the FINITE points that are not ground, the number of ground points): with extract_ground's result a partition of the finite points."""
    from .layout import PointAttributeDataType as T
    ground = _DeviceArray(buffer.api, T.U8, buffer.len())

    def fill(keep):  # finite, then cleared where ground
        count = ground_mask(buffer, params, device_mask_ptr=ground.ptr or 1)[1]
        finite_mask(buffer, keep.ptr)
        set_u8_where(keep.buffer, keep.attribute, ground.ptr, 0)
        return count
    return _filter_by_device_mask(buffer, out_buffer_type, fill, whole_array=True)


def _grid_morphology(op: int, device_in_ptr: int, device_out_ptr: int, cols: int, rows: int, half_width: int, api=None) -> None:
    from ._capi import product_api
    (api or product_api()).grid_morphology_device(C.c_void_p(int(device_in_ptr) or None), C.c_void_p(int(device_out_ptr) or None), cols, rows, half_width, op)


def grid_erode(device_in_ptr: int, device_out_ptr: int, cols: int, rows: int, half_width: int, api=None) -> None:
    """Stream-ordered, not in place: out[r][c] = the minimum of the float64 (rows, cols) raster at device_in_ptr over the square of half_width
    cells around (r, c), clipped to the raster.  Entries are finite or +inf."""
    _grid_morphology(0, device_in_ptr, device_out_ptr, cols, rows, half_width, api)


def grid_dilate(device_in_ptr: int, device_out_ptr: int, cols: int, rows: int, half_width: int, api=None) -> None:
    """As grid_erode, with the maximum over the entries below +inf (+inf where the square holds none)."""
    _grid_morphology(1, device_in_ptr, device_out_ptr, cols, rows, half_width, api)


def pmf_kernel_shape(api=None) -> dict:
    """The seams of the ground filter's kernels: points per workgroup of the point passes, columns and rows of a morphology tile, the largest
    half-width of one morphology pass."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(4)]
    (api or product_api()).pmf_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "tile_cols", "tile_rows", "max_half_width"), (x.value for x in v)))


def pmf_phase_times(api=None):
    """(bounds + raster, morphology, classification) in milliseconds of this thread's last ground_mask call; zeros unless PST_PMF_TIMES=1 was
    set when the library first ran one."""
    return _phase_times(api, "pmf_phase_times", 3)


# ---- nearest neighbours between two clouds, ICP (include/pasture_amd.h) ----------------------------------------------------------------------

NO_MATCH = 0xFFFFFFFF


def _transform12(transform):
    """A 3 x 4 [R | t] (or a 4 x 4 whose last row is 0 0 0 1) as 12 C doubles, row-major; None stays None."""
    if transform is None:
        return None
    t = np.asarray(transform, dtype=np.float64)
    if t.shape == (4, 4):
        if not np.array_equal(t[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of a 4 x 4 transform must be 0 0 0 1")
        t = t[:3]
    if t.shape != (3, 4):
        raise ValueError("a transform is a 3 x 4 or 4 x 4 array")
    return (C.c_double * 12)(*t.reshape(12))


class NearestNeighbourIndex:
    """The persistent nearest-neighbour index over `target` (pst_nn_index_create): a uniform grid over its finite points, kept in device memory
    of its own until destroy().  cell_edge = 0 chooses the edge from the cloud; the target buffer is not read after construction."""

    def __init__(self, target: _Buffer, cell_edge: float = 0.0):
        self.api = target.api
        self._h = None
        h = C.c_void_p()
        self.api.nn_index_create(target._h, cell_edge, C.byref(h))
        self._h = h

    def grid(self) -> dict:
        """origin (3,), the final cell edge, cells per axis (3,), the number of finite targets and of occupied cells."""
        me, dim, nf, occ = (C.c_double * 4)(), (C.c_uint32 * 3)(), C.c_uint64(), C.c_uint64()
        self.api.nn_index_grid(self._h, me, dim, C.byref(nf), C.byref(occ))
        return {"origin": tuple(me[0:3]), "cell_edge": me[3], "dim": tuple(dim), "n_finite": nf.value, "occupied_cells": occ.value}

    def set_normals(self, normals, n: Optional[int] = None) -> None:
        """The target's normals for icp_plane, kept in the index (in device memory of its own) and used as given: not normalised, not
        re-oriented.  `normals` is a buffer of the target's length with a NORMAL attribute (what compute_normals_into fills), or the address
        of f64 [n][3] in DEVICE memory in target-buffer order with its length `n` (what compute_normals_device writes), or None, which drops
        them.  Synchronous: the source is not read after the call; a later call replaces the normals."""
        if normals is None:
            self.api.nn_index_set_normals_device(self._h, None, 0)
        elif isinstance(normals, (int, np.integer)):
            if n is None or not normals:
                raise ValueError("a device address must not be 0 and needs the number of normals, n")
            self.api.nn_index_set_normals_device(self._h, C.c_void_p(int(normals)), n)
        else:
            self.api.nn_index_set_normals(self._h, normals._h)

    @property
    def has_normals(self) -> bool:
        out = C.c_int()
        self.api.nn_index_has_normals(self._h, C.byref(out))
        return bool(out.value)

    @classmethod
    def with_normals(cls, target: _Buffer, k_nn: int = 16, cell_edge: float = 0.0) -> "NearestNeighbourIndex":
        """The index over `target` with the normals compute_normals_device estimates from k_nn neighbours (their signs are arbitrary, which
        point-to-plane ICP does not mind); the temporary device array of the normals is released before this returns."""
        from .layout import PointAttributeDataType as T
        index = cls(target, cell_edge)
        try:
            n = target.len()
            normals = _DeviceArray(target.api, T.F64, 3 * n)
            compute_normals_device(target, k_nn, normals_ptr=normals.ptr)
            index.set_normals(normals.ptr, n)
        except Exception:
            index.destroy()
            raise
        return index

    def destroy(self) -> None:
        if self._h is not None and self._h.value:
            self.api.nn_index_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class _IndexFor:
    """`target_or_index` as an index: one that is passed in stays the caller's, one built here is destroyed on exit."""

    def __init__(self, target_or_index):
        self.own = not isinstance(target_or_index, NearestNeighbourIndex)
        self.index = NearestNeighbourIndex(target_or_index) if self.own else target_or_index

    def __enter__(self):
        return self.index

    def __exit__(self, *exc):
        if self.own:
            self.index.destroy()


def nearest_neighbours_device(query: _Buffer, index: NearestNeighbourIndex, max_distance: float = float("inf"), transform=None, idx_ptr: int = 0,
                              dist_ptr: int = 0) -> None:
    """For every point of `query` (sent through `transform` first, if given) the nearest finite target of `index` within max_distance, in
    caller-owned DEVICE memory (addresses; 0 = not wanted, not both): buffer indices uint32 [n] (NO_MATCH without one), distances f64 [n] (+inf)."""
    query.api.nearest_neighbours_device(index._h, query._h, _transform12(transform), max_distance, C.c_void_p(idx_ptr or None), C.c_void_p(dist_ptr or None))


def nearest_neighbours(query: _Buffer, target_or_index, max_distance: float = float("inf"), transform=None):
    """(idx uint32 (n,), dist float64 (n,)) as numpy arrays: the exact nearest neighbour of every query point in another cloud (a buffer, or a
    NearestNeighbourIndex built over it once and searched many times)."""
    from .layout import PointAttributeDataType as T
    n = query.len()
    idx, dist = _DeviceArray(query.api, T.U32, n), _DeviceArray(query.api, T.F64, n)
    with _IndexFor(target_or_index) as index:
        query.api.nearest_neighbours_device(index._h, query._h, _transform12(transform), max_distance, C.c_void_p(idx.ptr or 1), C.c_void_p(dist.ptr or 1))
    return idx.to_numpy(), dist.to_numpy()


def cloud_to_cloud_distances(query: _Buffer, target, max_distance: float = float("inf")) -> np.ndarray:
    """CloudCompare's C2C distance: per query point the distance to the nearest point of `target` (a buffer or an index), +inf beyond max_distance."""
    return nearest_neighbours(query, target, max_distance)[1]


def distance_mask(device_dist_ptr: int, n: int, threshold: float, keep_far: bool, device_mask_ptr: int, api=None) -> None:
    """Stream-ordered: mask[i] = 1 iff dist[i] <= threshold (keep_far: iff NOT dist[i] <= threshold, which holds for unmatched points), both arrays
    (n f64 / n bytes) in DEVICE memory -- the mask filter / filter_into take as (device_mask_ptr, 'device')."""
    from ._capi import product_api
    (api or product_api()).distance_mask_device(C.c_void_p(int(device_dist_ptr) or None), n, threshold, 1 if keep_far else 0, C.c_void_p(int(device_mask_ptr) or None))


def icp_step(index: NearestNeighbourIndex, source: _Buffer, transform, max_distance: float):
    """One point-to-point ICP step from `transform`: (sums (17,) = [m, cq xyz, cp xyz, H row-major, sum_d2], transform_out 3 x 4).
    sqrt(sums[16] / sums[0]) is the rms misfit of `transform`, not of transform_out."""
    sums, out = (C.c_double * 17)(), (C.c_double * 12)()
    source.api.icp_step(index._h, source._h, _transform12(transform), max_distance, sums, out)
    return np.array(sums, dtype=np.float64), np.array(out, dtype=np.float64).reshape(3, 4)


def icp(source: _Buffer, target_or_index, max_distance: float, max_iterations: int = 50, rms_tolerance: float = 0.0, init=None):
    """Point-to-point ICP of `source` onto a target (PDAL's filters.icp, PCL's IterativeClosestPoint): (transform 3 x 4, rms, matched, iterations).
    Stops after the step whose rms differs from the previous one's by at most rms_tolerance, or after max_iterations steps."""
    out, rms, matched, steps = (C.c_double * 12)(), C.c_double(), C.c_uint64(), C.c_uint32()
    with _IndexFor(target_or_index) as index:
        source.api.icp(index._h, source._h, _transform12(init), max_distance, max_iterations, rms_tolerance, out, C.byref(rms), C.byref(matched), C.byref(steps))
    return np.array(out, dtype=np.float64).reshape(3, 4), rms.value, matched.value, steps.value


def icp_plane_step(index: NearestNeighbourIndex, source: _Buffer, transform, max_distance: float):
    """One point-to-plane ICP step from `transform` on an index that has normals: (sums (35,) = [m, u, cq xyz, A (21: upper triangle of the
    6 x 6, row-major), g (6), sum_r2, sum_w2, sum_d2], transform_out 3 x 4).  sqrt(sums[32] / sums[1]) is the point-to-plane rms misfit of
    `transform`, not of transform_out."""
    sums, out = (C.c_double * 35)(), (C.c_double * 12)()
    source.api.icp_plane_step(index._h, source._h, _transform12(transform), max_distance, sums, out)
    return np.array(sums, dtype=np.float64), np.array(out, dtype=np.float64).reshape(3, 4)


def icp_plane(source: _Buffer, index: NearestNeighbourIndex, max_distance: float, max_iterations: int = 50, rms_tolerance: float = 0.0, init=None):
    """Point-to-plane ICP of `source` onto the target of `index` (PCL's IterativeClosestPointWithNormals, Open3D's
    TransformationEstimationPointToPlane): (transform 3 x 4, rms, used pairs, iterations), with the stopping rule of icp on the point-to-plane
    rms.  `index` must be a NearestNeighbourIndex that has normals (set_normals, or NearestNeighbourIndex.with_normals): a buffer in its place
    is refused with a TypeError, because how its normals are to be estimated (k_nn) is the caller's choice, not a default of the loop."""
    if not isinstance(index, NearestNeighbourIndex):
        raise TypeError("icp_plane needs a NearestNeighbourIndex with normals (NearestNeighbourIndex.with_normals(target, k_nn)), not a buffer")
    out, rms, used, steps = (C.c_double * 12)(), C.c_double(), C.c_uint64(), C.c_uint32()
    source.api.icp_plane(index._h, source._h, _transform12(init), max_distance, max_iterations, rms_tolerance, out, C.byref(rms), C.byref(used), C.byref(steps))
    return np.array(out, dtype=np.float64).reshape(3, 4), rms.value, used.value, steps.value


def nn_kernel_shape(api=None) -> dict:
    """The seams of the nearest-neighbour kernels: queries one workgroup of the search owns, threads of the workgroup that adds the block partials
    of the ICP sums, source points per block partial."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).nn_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("queries_per_block", "reduce_block", "reduce_points_per_block"), (x.value for x in v)))


def nn_phase_times(api=None):
    """(query keys + sort, search) in milliseconds of this thread's last nearest_neighbours* call; zeros unless PST_NN_TIMES=1 was set when the
    library first ran one."""
    return _phase_times(api, "nn_phase_times", 2)


# ---- M3C2 change detection: signed distances along normals (include/pasture_amd.h) --------------------------------------------------------------

M3C2_ORIENT_UP = 1


@dataclass
class M3C2Result:
    """Per core point: the signed distance from the reference to the compared cloud along the normal, its 95 % level of detection, whether
    |distance| exceeds it, the members of the two cylinders (n, 2) and their spreads sqrt(var_X) (n, 2); n_significant = significant.sum().
    NaN where a figure is not defined (too few members, an invalid core point).  sums (n, 4) = St_1, Stt_1, St_2, Stt_2 and unit_normals
    (n, 3) with return_sums."""
    distance: np.ndarray
    lod: np.ndarray
    significant: np.ndarray
    counts: np.ndarray
    spread: np.ndarray
    n_significant: int
    sums: Optional[np.ndarray] = None
    unit_normals: Optional[np.ndarray] = None


def m3c2_device(core: _Buffer, reference: NearestNeighbourIndex, compared: NearestNeighbourIndex, radius: float, max_depth: float, normals_ptr: int = 0,
                min_points: int = 4, registration_error: float = 0.0, orient_up: bool = False, distance_ptr: int = 0, lod_ptr: int = 0, significant_ptr: int = 0,
                counts_ptr: int = 0, sums_ptr: int = 0, unit_normals_ptr: int = 0, count_significant: bool = True) -> Optional[int]:
    """M3C2 of the core points against two indexed clouds, results in caller-owned DEVICE memory (addresses; 0 = not wanted): distance and lod
    f64 [n], significant u8 [n], counts u32 [n][2], sums f64 [n][4], unit normals f64 [n][3].  normals_ptr: f64 [n][3] in core order on the
    device, or 0 for the normal `reference` holds for the nearest reference point.  Nothing is copied; returns the number of significant core
    points (None with count_significant=False)."""
    nsig = C.c_uint64()
    core.api.m3c2_device(reference._h, compared._h, core._h, C.c_void_p(normals_ptr or None), radius, max_depth, min_points, registration_error,
                         M3C2_ORIENT_UP if orient_up else 0, C.c_void_p(distance_ptr or None), C.c_void_p(lod_ptr or None), C.c_void_p(significant_ptr or None),
                         C.c_void_p(counts_ptr or None), C.c_void_p(sums_ptr or None), C.c_void_p(unit_normals_ptr or None), C.byref(nsig) if count_significant else None)
    return nsig.value if count_significant else None


class _NormalIndexFor(_IndexFor):
    """_IndexFor whose own index carries the normals compute_normals_device estimates (NearestNeighbourIndex.with_normals)"""

    def __init__(self, target_or_index, k_nn: int):
        self.own = not isinstance(target_or_index, NearestNeighbourIndex)
        self.index = NearestNeighbourIndex.with_normals(target_or_index, k_nn) if self.own else target_or_index


def m3c2(core: _Buffer, reference, compared, radius: float, max_depth: float, normals=None, min_points: int = 4, registration_error: float = 0.0,
         orient_up: bool = False, return_sums: bool = False, k_nn: int = 16) -> M3C2Result:
    """M3C2 (Lague, Brodu & Leroux 2013; CloudCompare's plugin, py4dgeo): per core point the signed distance between two aligned clouds along the
    local normal, from the points of each cloud inside a cylinder of `radius` reaching `max_depth` to either side, with the 95 % level of
    detection 1.96 * (sqrt(var_1/n_1 + var_2/n_2) + registration_error).  `reference` and `compared` are buffers or NearestNeighbourIndex
    objects; `normals` is the address of f64 [n][3] on the device, a host array (n, 3), or None: the normal of the nearest reference point,
    for which a `reference` given as a buffer is indexed with NearestNeighbourIndex.with_normals(reference, k_nn)."""
    from .layout import PointAttributeDataType as T
    api, n = core.api, core.len()
    nptr, keep = _device_input(api, normals, T.F64, np.float64, 3 * n, "normals")
    dist, lod, sig = _DeviceArray(api, T.F64, n), _DeviceArray(api, T.F64, n), _DeviceArray(api, T.U8, n)
    counts, sums = _DeviceArray(api, T.U32, 2 * n), _DeviceArray(api, T.F64, 4 * n)
    unit = _DeviceArray(api, T.F64, 3 * n) if return_sums else None
    with (_NormalIndexFor(reference, k_nn) if normals is None else _IndexFor(reference)) as ref, _IndexFor(compared) as cmp:
        nsig = m3c2_device(core, ref, cmp, radius, max_depth, nptr, min_points, registration_error, orient_up, dist.ptr or 1, lod.ptr or 1, sig.ptr or 1,
                           counts.ptr or 1, sums.ptr or 1, unit.ptr or 1 if unit else 0)
    del keep
    c = counts.to_numpy().reshape(n, 2)
    s = sums.to_numpy().reshape(n, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = c.astype(np.float64)
        q = s[:, 1::2] - (s[:, 0::2] * s[:, 0::2]) / m
        spread = np.sqrt(np.where(q > 0.0, q, 0.0) / (c.astype(np.int64) - 1))
    spread[c < 2] = np.nan
    return M3C2Result(dist.to_numpy(), lod.to_numpy(), sig.to_numpy().astype(bool), c, spread, nsig, s if return_sums else None,
                      unit.to_numpy().reshape(n, 3) if unit else None)


def m3c2_kernel_shape(api=None) -> dict:
    """The seams of the M3C2 kernel: core points one workgroup owns, lanes that share one core point."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).m3c2_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("cores_per_block", "lanes_per_core"), (x.value for x in v)))


def m3c2_phase_times(api=None):
    """(normal lookup, core keys + sort, cylinder pass) in milliseconds of this thread's last m3c2* call; zeros unless PST_M3C2_TIMES=1 was set
    when the library first ran one."""
    return _phase_times(api, "m3c2_phase_times", 3)


def m3c2_work(api=None) -> dict:
    """rows of cells searched, candidates tested and members found by this thread's last m3c2* call, over both clouds; zeros unless
    PST_M3C2_WORK=1 was set when the library first ran one."""
    from ._capi import product_api
    out = (C.c_uint64 * 3)()
    (api or product_api()).m3c2_work(out)
    return dict(zip(("rows", "candidates", "members"), (int(x) for x in out)))


# ---- height above ground from the k nearest ground points in the XY plane (include/pasture_amd.h) ---------------------------------------------

def classification_mask(buffer: _Buffer, value: int, device_mask_ptr: int) -> None:
    """Stream-ordered: len(buffer) bytes in DEVICE memory, 1 where the LAS Classification (U8) equals `value` -- the inverse of what
    classify_ground writes, and the ground mask of height_above_ground without a host round trip."""
    from .layout import attributes as A
    buffer.api.buffer_u8_equals_mask_device(buffer._h, A.CLASSIFICATION.name().encode(), value, C.c_void_p(int(device_mask_ptr) or None))


def height_above_ground_device(buffer: _Buffer, device_ground_mask_ptr: Optional[int] = None, k: int = 1, max_distance: float = float("inf"), ground: Optional[_Buffer] = None,
                               cell_edge: float = 0.0, hag_ptr: int = 0, ground_z_ptr: int = 0) -> dict:
    """PDAL's filters.hag_nn on the device: for every point of `buffer` the elevation of the ground under it -- the inverse squared distance
    weighted mean of the z of its k nearest ground points IN THE XY PLANE within max_distance -- and its height above it, as float64 in
    caller-owned DEVICE memory (addresses; 0 = not wanted, not both).  The ground points are those of `ground` (None: `buffer` itself) whose
    byte in the DEVICE mask at device_ground_mask_ptr is not zero (None or 0: every finite point of it).  Returns {"n_ground",
    "n_unresolved" (finite points without a ground point in reach: NaN), "origin", "cell_edge", "dim"} -- the last three describe the grid
    that was used, which the result does not depend on."""
    ng, nu, me, dim = C.c_uint64(), C.c_uint64(), (C.c_double * 3)(), (C.c_uint32 * 2)()
    g = buffer if ground is None else ground
    buffer.api.height_above_ground_device(buffer._h, g._h, C.c_void_p(int(device_ground_mask_ptr or 0) or None), k, max_distance, cell_edge, C.c_void_p(hag_ptr or None),
                                          C.c_void_p(ground_z_ptr or None), C.byref(ng), C.byref(nu), me, dim)
    return {"n_ground": ng.value, "n_unresolved": nu.value, "origin": (me[0], me[1]), "cell_edge": me[2], "dim": (dim[0], dim[1])}


def _ground_mask_array(buffer: _Buffer, ground: Optional[_Buffer], ground_mask):
    """(the _DeviceArray that keeps an uploaded or computed mask alive, or None; the mask's device address, or None)"""
    from .layout import PointAttributeDataType as T
    g = buffer if ground is None else ground
    if ground_mask is None:  # Classification == 2
        held = _DeviceArray(g.api, T.U8, g.len())
        classification_mask(g, 2, held.ptr)
        return held, held.ptr
    if isinstance(ground_mask, (int, np.integer)):
        return None, int(ground_mask)
    m = np.ascontiguousarray(ground_mask, dtype=np.uint8)
    if m.shape != (g.len(),):
        raise ValueError("ground_mask must have one byte per point of the ground buffer")
    held = _DeviceArray(g.api, T.U8, g.len())
    if g.len():
        held.buffer.set_attribute_range(held.attribute, range(0, g.len()), m)
    return held, held.ptr


def height_above_ground(buffer: _Buffer, ground_mask=None, k: int = 1, max_distance: float = float("inf"), ground: Optional[_Buffer] = None, cell_edge: float = 0.0,
                        return_ground_z: bool = False):
    """Height above ground of every point of `buffer` as numpy float64 (n,), or (hag, ground_z) with return_ground_z: see
    height_above_ground_device.  ground_mask: a numpy uint8 array with one byte per point of the ground buffer (uploaded), the address of
    such bytes in DEVICE memory, or None for Classification == 2 (what classify_ground writes).  ground = None: the buffer itself.  Points
    without a ground point within max_distance, and points that are not finite, get NaN."""
    from .layout import PointAttributeDataType as T
    n = buffer.len()
    held, mask_ptr = _ground_mask_array(buffer, ground, ground_mask)
    hag = _DeviceArray(buffer.api, T.F64, n)
    gz = _DeviceArray(buffer.api, T.F64, n) if return_ground_z else None
    height_above_ground_device(buffer, mask_ptr, k, max_distance, ground, cell_edge, hag.ptr or 1, (gz.ptr or 1) if gz else 0)
    del held
    return (hag.to_numpy(), gz.to_numpy()) if return_ground_z else hag.to_numpy()


def normalize_height(buffer: _Buffer, ground_mask=None, k: int = 1, max_distance: float = float("inf"), ground: Optional[_Buffer] = None, cell_edge: float = 0.0) -> int:
    """lidR's normalize_height(knnidw()): replaces the z of every Position3D of `buffer` IN PLACE by its height above ground, computed and
    written on the device (x and y keep their bits).  Returns n_unresolved: that many finite points had no ground point within
    max_distance; their z, like that of every point that is not finite, becomes NaN.  With the buffer as its own ground the ground mask is
    taken BEFORE z changes; the ground points themselves end at height +0.0."""
    from .layout import PointAttributeDataType as T, attributes as A
    n = buffer.len()
    held, mask_ptr = _ground_mask_array(buffer, ground, ground_mask)
    hag = _DeviceArray(buffer.api, T.F64, n)
    info = height_above_ground_device(buffer, mask_ptr, k, max_distance, ground, cell_edge, hag.ptr or 1)
    if n:
        transform_attribute_expr(buffer, A.POSITION_3D, "x ; y ; p0[i]", [hag.ptr])
        buffer.api.stream_synchronize()  # (the heights are released when this returns)
    del held
    return info["n_unresolved"]


def hag_kernel_shape(api=None) -> dict:
    """The seams of the height-above-ground kernels: queries one workgroup of the search owns, the largest k, ground points per block partial
    of the masked bounds."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).hag_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("queries_per_block", "max_k", "bounds_points_per_block"), (x.value for x in v)))


def hag_phase_times(api=None):
    """(ground bounds + keys + sort + directory, query keys + sort, search) in milliseconds of this thread's last height_above_ground* call;
    zeros unless PST_HAG_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "hag_phase_times", 3)


# ---- rasterisation: per-cell statistics on an XY grid, and the hole filler (include/pasture_amd.h) --------------------------------------------

RASTER_STATS = {"count": 1, "min": 2, "max": 4, "mean": 8, "variance": 16}  # plane name -> bit of `stats`; the planes come in ascending bit order


@dataclass(frozen=True)
class Raster:
    """What rasterize returns: the grid that was used -- origin (x0, y0), cell_size, cols, rows; zeros for a cloud without a finite point --,
    the number of members, and `planes`: statistic name -> float64 (rows, cols) array (empty when the planes went to device memory)."""
    origin: Tuple[float, float]
    cell_size: float
    cols: int
    rows: int
    n_members: int
    planes: dict


def _values_column(buffer: _Buffer, attribute: PointAttributeDefinition):
    """the scalar attribute of every point as a float64 device column (a _DeviceArray), through the layout converter"""
    from .conversion import BufferLayoutConverter
    from .layout import PointAttributeDataType as T
    column = _DeviceArray(buffer.api, T.F64, buffer.len())
    if buffer.len():
        converter = BufferLayoutConverter.for_layouts_with_default(buffer.point_layout(), column.buffer.point_layout())
        converter.set_custom_mapping(attribute, column.attribute)
        converter.convert_into(buffer, column.buffer)
    return column


def rasterize(buffer: _Buffer, cell_size: float, stats=("max",), values=None, device_mask_ptr: Optional[int] = None, origin=None, dim=None,
              device_out_ptr: Optional[int] = None) -> Raster:
    """Per-cell statistics of a cloud on an XY grid, on the device: `stats` names planes of "count", "min", "max", "mean", "variance" and
    "stdev" (the square root of the variance plane, taken on the host: host results only).  values: None for z, the address of len(buffer)
    float64 in DEVICE memory (the heights of height_above_ground_device), or a scalar attribute of the buffer (converted to a float64
    device column).  device_mask_ptr: one byte per point in DEVICE memory, only points with a non-zero byte take part.  origin = (x0, y0)
    and dim = (cols, rows) together: that grid; neither: pmf_grid's, whatever the mask.  device_out_ptr: the planes go to DEVICE memory
    there, float64 [planes][rows][cols] in the order count, min, max, mean, variance, and Raster.planes is empty -- the caller sizes it from
    pmf_grid or the given dim.  An empty cell has count 0 and NaN in every other plane.  (Host planes on the automatic grid cost one
    pmf_grid call first, to size the arrays.)"""
    names = [stats] if isinstance(stats, str) else list(stats)
    unknown = [s for s in names if s not in RASTER_STATS and s != "stdev"]
    if unknown:
        raise ValueError(f"unknown statistics {unknown}: choose from {sorted(RASTER_STATS)} and 'stdev'")
    if device_out_ptr is not None and "stdev" in names:
        raise ValueError("'stdev' is computed on the host: ask for 'variance' with device_out_ptr")
    bits = 0
    for s in names:
        bits |= RASTER_STATS["variance" if s == "stdev" else s]
    if (origin is None) != (dim is None):
        raise ValueError("origin and dim must be given together or not at all")
    held = None
    if isinstance(values, PointAttributeDefinition):
        held = _values_column(buffer, values)
        values_ptr = held.ptr
    else:
        values_ptr = int(values) if values is not None else 0
    c_origin = (C.c_double * 2)(*origin) if origin is not None else None
    c_dim = (C.c_uint32 * 2)(*dim) if dim is not None else None
    origin_out, dim_out, members = (C.c_double * 2)(), (C.c_uint32 * 2)(), C.c_uint64()
    planes_of = [name for name, bit in RASTER_STATS.items() if bits & bit]
    host = None
    if device_out_ptr is None:
        if dim is not None:
            cols, rows = int(dim[0]), int(dim[1])
        else:
            grid = pmf_grid(buffer, cell_size)
            cols, rows = grid["cols"], grid["rows"]
        host = np.full((max(len(planes_of), 1), rows, cols), np.nan, dtype=np.float64)
        out_ptr, memkind = C.c_void_p(host.ctypes.data if host.size else 1), 1
    else:
        out_ptr, memkind = C.c_void_p(int(device_out_ptr) or None), 0
    buffer.api.rasterize(buffer._h, C.c_void_p(values_ptr or None), C.c_void_p(int(device_mask_ptr or 0) or None), cell_size, c_origin, c_dim, bits, out_ptr, memkind,
                         origin_out, dim_out, C.byref(members))
    del held
    planes = {}
    if host is not None:
        by_name = dict(zip(planes_of, host))
        planes = {s: (np.sqrt(by_name["variance"]) if s == "stdev" else by_name[s]) for s in names}
    return Raster((origin_out[0], origin_out[1]), cell_size, dim_out[0], dim_out[1], members.value, planes)


def grid_fill(device_in_ptr: int, device_out_ptr: int, cols: int, rows: int, half_width: int, api=None) -> None:
    """Stream-ordered, not in place: the float64 (rows, cols) raster at device_in_ptr with every entry that is not finite (the NaN of
    rasterize, the +inf of the ground filter's surfaces) replaced by the inverse-squared-distance weighted mean of the finite entries within
    half_width cells (at most 16) of it, NaN where there is none; finite entries keep their bits."""
    from ._capi import product_api
    (api or product_api()).grid_fill_device(C.c_void_p(int(device_in_ptr) or None), C.c_void_p(int(device_out_ptr) or None), cols, rows, half_width)


def raster_kernel_shape(api=None) -> dict:
    """The seams of the rasterisation kernels: points per workgroup of the atomic pass, the chunk length of the sums (part of the definition),
    columns and rows of a fill tile, the largest fill half-width."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(5)]
    (api or product_api()).raster_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "chunk", "fill_tile_cols", "fill_tile_rows", "fill_max_half_width"), (x.value for x in v)))


def raster_phase_times(api=None):
    """(bounds, keys + sort + directory, reduction + output) in milliseconds of this thread's last rasterize call; zeros unless
    PST_RASTER_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "raster_phase_times", 3)


# ---- geometric features from the eigenvalues of the neighbourhood covariance (include/pasture_amd.h) -----------------------------------------

# plane name -> bit of `features`; the planes come in ascending bit order
FEATURES = {"eigenvalue_1": 1, "eigenvalue_2": 2, "eigenvalue_3": 4, "linearity": 8, "planarity": 16, "scattering": 32, "anisotropy": 64,
            "surface_variation": 128, "eigenvalue_sum": 256, "verticality": 512, "omnivariance": 1024, "eigenentropy": 2048, "count": 4096}


def _feature_bits(features) -> int:
    if isinstance(features, (int, np.integer)):
        return int(features)
    names = [features] if isinstance(features, str) else list(features)
    unknown = [s for s in names if s not in FEATURES]
    if unknown:
        raise ValueError(f"unknown features {unknown}: choose from {list(FEATURES)}")
    bits = 0
    for s in names:
        bits |= FEATURES[s]
    return bits


def geometric_features_device(buffer: _Buffer, k: int, features, out_ptr: int, max_distance: float = float("inf"), normals_ptr: int = 0, directions_ptr: int = 0,
                              knn_ptr: int = 0, from_knn: bool = False) -> None:
    """Per-point features of the covariance of the k nearest neighbours, everything in caller-owned DEVICE memory: out_ptr float64 [planes][n],
    one plane per feature (names of FEATURES, or their bits) in ascending bit order; normals_ptr / directions_ptr float64 [n][3], the
    eigenvectors of the smallest / largest eigenvalue, oriented upwards; 0 = not wanted, but one of the three is needed.  knn_ptr: uint32
    [n][k].  from_knn=False: the library searches (k = 3 .. 64) and, if knn_ptr is given, leaves its lists there; synchronous.
    from_knn=True: the lists at knn_ptr are the input (k = 1 .. 64; indices >= n are skipped); stream-ordered, no synchronisation.
    Only neighbours within max_distance of the query take part."""
    p = lambda a: C.c_void_p(int(a) or None)  # noqa: E731
    if from_knn:
        buffer.api.geometric_features_from_knn_device(buffer._h, k, p(knn_ptr), max_distance, _feature_bits(features), p(out_ptr), p(normals_ptr), p(directions_ptr))
    else:
        buffer.api.geometric_features(buffer._h, k, max_distance, _feature_bits(features), p(out_ptr), p(normals_ptr), p(directions_ptr), p(knn_ptr))


def geometric_features(buffer: _Buffer, k: int, features=("linearity", "planarity", "scattering", "verticality"), max_distance: float = float("inf"), knn=None,
                       return_normals: bool = False, return_directions: bool = False) -> dict:
    """PDAL's filters.covariancefeatures / CloudCompare's geometric features on the device: a dict from feature name (FEATURES) to a float64
    (n,) array, with "normals" / "directions" (n, 3) when asked for.  knn: an optional (n, k) integer array of neighbour indices (-1 or
    anything >= n: no neighbour), as knn_search returns it; without it the library searches the k nearest neighbours itself.  A point with
    fewer than 3 valid neighbours has NaN everywhere but in "count"."""
    from .layout import PointAttributeDataType as T
    names = [features] if isinstance(features, str) else list(features)
    bits = _feature_bits(names)
    planes_of = [name for name, bit in FEATURES.items() if bits & bit]
    n = buffer.len()
    lists = None
    if knn is not None:
        knn = np.asarray(knn)
        if knn.ndim != 2 or knn.shape != (n, k) or knn.dtype.kind not in "iu":
            raise ValueError("knn must be an integer array of shape (len(buffer), k)")
        lists = _DeviceArray(buffer.api, T.U32, n * k)
        if n * k:
            lists.buffer.set_attribute_range(lists.attribute, range(0, n * k), (knn.astype(np.int64).reshape(-1) & 0xFFFFFFFF).astype(np.uint32))
    out = _DeviceArray(buffer.api, T.F64, n * len(planes_of))
    normals = _DeviceArray(buffer.api, T.F64, n * 3) if return_normals else None
    directions = _DeviceArray(buffer.api, T.F64, n * 3) if return_directions else None
    # (an empty array has no address: the calls' own checks answer such a buffer before anything is dereferenced)
    geometric_features_device(buffer, k, bits, out.ptr or (1 if planes_of else 0), max_distance, (normals.ptr or 1) if normals else 0,
                              (directions.ptr or 1) if directions else 0, (lists.ptr or 1) if lists else 0, from_knn=lists is not None)
    if lists is not None:
        buffer.api.stream_synchronize()
    result = dict(zip(planes_of, out.to_numpy().reshape(len(planes_of), n)))
    result = {s: result[s] for s in names}
    if normals:
        result["normals"] = normals.to_numpy().reshape(n, 3)
    if directions:
        result["directions"] = directions.to_numpy().reshape(n, 3)
    return result


def features_kernel_shape(k: int, api=None) -> dict:
    """The seams of the feature kernel at this k: points whose whole neighbour lists one workgroup owns, and its threads."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).features_kernel_shape(k, *[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "threads"), (x.value for x in v)))


# ---- minimum-distance (Poisson-disk) subsampling (include/pasture_amd.h) ---------------------------------------------------------------------

SAMPLE_ORDERS = {"shuffled": 0, "index": 1}


def _sample_order(order) -> int:
    if order not in SAMPLE_ORDERS:
        raise ValueError(f"order must be one of {sorted(SAMPLE_ORDERS)}")
    return SAMPLE_ORDERS[order]


def sample_priorities(order, seed: int, first: int, count: int, api=None) -> np.ndarray:
    """The priority keys of buffer indices first .. first + count - 1 (host only): splitmix64(seed ^ i) for "shuffled", i for "index"."""
    from ._capi import product_api
    keys = np.zeros(count, dtype=np.uint64)
    (api or product_api()).sample_priorities(_sample_order(order), seed & 0xFFFFFFFFFFFFFFFF, first & 0xFFFFFFFFFFFFFFFF, count, _u64(keys) if count else None)
    return keys


def poisson_disk_mask(buffer: _Buffer, radius: float, seed: int = 0, order: str = "shuffled", device_mask_ptr: Optional[int] = None):
    """PDAL's filters.sample / CloudCompare's "subsample by space" on the device: the greedy pass in ascending priority key that keeps a finite
    point iff no kept point lies within `radius` of it.  order "shuffled": keys splitmix64(seed ^ index); "index": the buffer order itself
    (the first point is always kept; slow on scan-line ordered clouds).  Returns (mask, kept, rounds): mask is a numpy uint8 array (1 = keep),
    or None when the bytes went to DEVICE memory at device_mask_ptr -- what filter takes as (ptr, 'device'); rounds = launches of the decision
    kernel."""
    n = buffer.len()
    kept, rounds = C.c_uint64(), C.c_uint32()
    mask = np.zeros(n, dtype=np.uint8) if device_mask_ptr is None else None
    ptr = C.c_void_p(int(device_mask_ptr) or None) if mask is None else C.c_void_p(mask.ctypes.data if n else 1)
    buffer.api.poisson_disk_mask(buffer._h, radius, _sample_order(order), seed & 0xFFFFFFFFFFFFFFFF, ptr, 0 if mask is None else 1, C.byref(kept), C.byref(rounds))
    return mask, kept.value, rounds.value


def subsample_min_distance(buffer: _Buffer, radius: float, seed: int = 0, order: str = "shuffled", out_buffer_type=None):
    """(the points poisson_disk_mask keeps, in buffer order with all their attributes; their number): mask and compaction stay in device
    memory.  `buffer` is columnar (filter is defined on HashMapBuffer)."""
    return _filter_by_device_mask(buffer, out_buffer_type, lambda p: poisson_disk_mask(buffer, radius, seed, order, device_mask_ptr=p or 1)[1])


def sample_kernel_shape(api=None) -> dict:
    """The seams of the decision kernel: active points one workgroup owns, sweeps of a lane over its point per launch."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).sample_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "sweeps_per_launch"), (x.value for x in v)))


def sample_phase_times(api=None):
    """(index build, decision rounds, mask write) in milliseconds of this thread's last poisson_disk_mask call; zeros unless
    PST_SAMPLE_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "sample_phase_times", 3)


# ---- gather by index and sort orders: attribute, Morton, shuffle (include/pasture_amd.h) ----------------------------------------------------

def _order_result(api, n: int, device_order_ptr, call):
    """call(address of n u32) fills the order: into the caller's device memory (returns None), or into a numpy uint32 array"""
    from .layout import PointAttributeDataType as T
    if device_order_ptr is not None:
        call(C.c_void_p(int(device_order_ptr) or None))
        return None
    out = _DeviceArray(api, T.U32, n)
    call(C.c_void_p(out.ptr or (None if n else 1)))
    return out.to_numpy()


def argsort_attribute(buffer: _Buffer, attribute: PointAttributeDefinition, component: int = 0, descending: bool = False, device_order_ptr: Optional[int] = None):
    """np.argsort(values, kind="stable") of one numeric attribute (component 0 .. 2 of a Vec3 one) on the device: NaNs last, ties in input
    order in both directions.  Returns a numpy uint32 array, or None when the order went to DEVICE memory at device_order_ptr."""
    cdt = attribute.datatype().to_c()
    return _order_result(buffer.api, buffer.len(), device_order_ptr,
                         lambda p: buffer.api.sort_order_by_attribute_device(buffer._h, attribute.name().encode(), C.byref(cdt), component, 1 if descending else 0, p))


def morton_order(buffer: _Buffer, dims: int = 3, bits: int = 0, device_order_ptr: Optional[int] = None, return_keys: bool = False):
    """The Z-order of the cloud (PDAL's filters.mortonorder with dims=2): `bits` per axis over the AABB of the finite points (0: 21 for three
    axes, 31 for two); points with a coordinate that is not finite come last.  Returns the order as argsort_attribute does; with return_keys
    (order, keys): the uint64 key of every point."""
    from .layout import PointAttributeDataType as T
    keys = _DeviceArray(buffer.api, T.U64, buffer.len()) if return_keys else None
    order = _order_result(buffer.api, buffer.len(), device_order_ptr,
                          lambda p: buffer.api.morton_order_device(buffer._h, dims, bits, p, C.c_void_p(keys.ptr or None) if keys else None))
    return (order, keys.to_numpy()) if return_keys else order


def shuffle_order(n: int, seed: int, device_order_ptr: Optional[int] = None, api=None):
    """The permutation that sorts 0 .. n - 1 by splitmix64(seed ^ i): the argsort of sample_priorities("shuffled", seed, 0, n)."""
    from ._capi import product_api
    api = api or product_api()
    return _order_result(api, n, device_order_ptr, lambda p: api.shuffle_order_device(n, seed & 0xFFFFFFFFFFFFFFFF, p))


def invert_order(order, device_inverse_ptr: Optional[int] = None, api=None):
    """inverse[order[j]] = j: a per-point result computed on a reordered cloud is carried back with result[inverse].  `order`: a numpy
    array, or a (device_ptr, n) pair."""
    from ._capi import product_api
    from .layout import PointAttributeDataType as T
    api = api or product_api()
    staged = None
    if isinstance(order, tuple):
        ptr, n = int(order[0]), int(order[1])
    else:
        order = np.ascontiguousarray(order, dtype=np.uint32)
        n = order.size
        staged = _DeviceArray(api, T.U32, n)
        if n:
            staged.buffer.set_attribute_range(staged.attribute, range(0, n), order)
        ptr = staged.ptr
    result = _order_result(api, n, device_inverse_ptr, lambda p: api.invert_order_device(C.c_void_p(ptr or None), n, p))
    if staged is not None and device_inverse_ptr is not None:
        api.stream_synchronize()  # the staged copy of the order is released on return
    return result


def _take_by_device_order(buffer: _Buffer, out_buffer_type, fill, return_order: bool = False):
    """fill(address of len(buffer) u32) writes an order; the points in that order, the list never leaving the device"""
    from .layout import PointAttributeDataType as T
    n = buffer.len()
    order = _DeviceArray(buffer.api, T.U32, n)
    result = fill(order.ptr or 1)
    out = buffer.take((order.ptr, n, 32), out_buffer_type)
    return (out, order.to_numpy(), result) if return_order else (out, None, result)


def sort_by_attribute(buffer: _Buffer, attribute: PointAttributeDefinition, component: int = 0, descending: bool = False, out_buffer_type=None):
    """PDAL's filters.sort: a new buffer with the points in argsort_attribute's order."""
    return _take_by_device_order(buffer, out_buffer_type, lambda p: argsort_attribute(buffer, attribute, component, descending, device_order_ptr=p))[0]


def morton_sort(buffer: _Buffer, dims: int = 3, bits: int = 0, out_buffer_type=None, return_order: bool = False):
    """A new buffer with the points in morton_order's order; with return_order (buffer, order)."""
    out, order, _ = _take_by_device_order(buffer, out_buffer_type, lambda p: morton_order(buffer, dims, bits, device_order_ptr=p), return_order)
    return (out, order) if return_order else out


def shuffle(buffer: _Buffer, seed: int, out_buffer_type=None):
    """PDAL's filters.randomize with a seed: a new buffer with the points in shuffle_order(len(buffer), seed)."""
    return _take_by_device_order(buffer, out_buffer_type, lambda p: shuffle_order(buffer.len(), seed, device_order_ptr=p, api=buffer.api))[0]


def reorder_kernel_shape(api=None) -> dict:
    """The seams of the gather kernel: consecutive output points one workgroup owns, bytes of its LDS record tile."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(2)]
    (api or product_api()).reorder_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "record_tile_bytes"), (x.value for x in v)))


def reorder_phase_times(api=None):
    """(bounds and keys, sort, gather) in milliseconds of this thread's last synchronous gather or sort-order call; zeros unless
    PST_REORDER_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "reorder_phase_times", 3)


# ---- polygon crop and overlay: point-in-polygon ids and masks (include/pasture_amd.h) ----------------------------------------------------------

NO_POLYGON = 0xFFFFFFFF
_CROP_KERNELS = {"auto": 0, "flat": 1, "banded": 2}


def _polygon_arrays(polygons):
    """`polygons` as the C ABI takes a set: vertices (V, 2) float64, ring offsets (R + 1,) uint64, polygon of every ring (R,) uint32"""
    rings, polygon_of_ring = [], []
    for p, polygon in enumerate(polygons):
        try:
            a = np.asarray(polygon, dtype=np.float64)
        except ValueError:  # rings of different lengths
            a = None
        parts = [a] if a is not None and a.ndim == 2 else [np.asarray(r, dtype=np.float64) for r in polygon]
        for ring in parts:
            if ring.ndim != 2 or ring.shape[1] != 2:
                raise ValueError("a ring is an (m, 2) array of x and y")
            rings.append(ring)
            polygon_of_ring.append(p)
    if not rings:
        raise ValueError("a polygon set has at least one polygon")
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.uint64)
    return np.ascontiguousarray(np.concatenate(rings)), offsets, np.asarray(polygon_of_ring, dtype=np.uint32)


class PolygonSet:
    """A set of polygons indexed for the point-in-polygon kernels (pst_polygon_set_create), in device memory of its own until destroy().
    `polygons` is a list of polygons; each is an (m, 2) array of x and y, or a list of such arrays -- outer rings and holes alike: ring
    orientation carries no meaning, the even-odd rule decides.  bands = 0 chooses the number of y-bands from the set; kernel is "auto",
    "flat" (every edge in LDS; small sets only) or "banded"."""

    def __init__(self, polygons, bands: int = 0, kernel: str = "auto", api=None):
        from ._capi import product_api
        self.api = api or product_api()
        self._h = None
        xy, offsets, polygon_of_ring = _polygon_arrays(polygons)
        h = C.c_void_p()
        self.api.polygon_set_create(xy.ctypes.data_as(C.POINTER(C.c_double)), _u64(offsets), len(offsets) - 1, polygon_of_ring.ctypes.data_as(C.POINTER(C.c_uint32)), bands,
                                    _CROP_KERNELS[kernel], C.byref(h))
        self._h = h

    @property
    def info(self) -> dict:
        """polygons, entries (the edges that are not horizontal), bands, directory_entries (entries summed over the bands that list them), the
        box (xmin, ymin, xmax, ymax) and the kernel taken."""
        counts, box, kernel = (C.c_uint64 * 4)(), (C.c_double * 4)(), C.c_uint32()
        self.api.polygon_set_info(self._h, counts, box, C.byref(kernel))
        return {"polygons": counts[0], "entries": counts[1], "bands": counts[2], "directory_entries": counts[3], "box": tuple(box),
                "kernel": {1: "flat", 2: "banded"}[kernel.value]}

    def destroy(self) -> None:
        if self._h is not None and self._h.value:
            self.api.polygon_set_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class _SetFor:
    """`polygons` as a PolygonSet: one that is passed in stays the caller's, one built here is destroyed on exit."""

    def __init__(self, polygons, api):
        self.own = not isinstance(polygons, PolygonSet)
        self.set = PolygonSet(polygons, api=api) if self.own else polygons

    def __enter__(self):
        return self.set

    def __exit__(self, *exc):
        if self.own:
            self.set.destroy()


def points_in_polygons(buffer: _Buffer, polygons, device_ids_ptr: Optional[int] = None):
    """Per point the smallest index of a polygon of the set that contains it (even-odd rule, half-open like the raster's cells; x and y only),
    NO_POLYGON = 0xFFFFFFFF without one.  `polygons` is a PolygonSet or what PolygonSet takes.  Returns a numpy uint32 array, or None when
    the len(buffer) values went to DEVICE memory at device_ids_ptr (stream-ordered then)."""
    from .layout import PointAttributeDataType as T
    with _SetFor(polygons, buffer.api) as ps:
        if device_ids_ptr is not None:
            buffer.api.points_in_polygons_device(ps._h, buffer._h, C.c_void_p(int(device_ids_ptr) or None))
            return None
        ids = _DeviceArray(buffer.api, T.U32, buffer.len())
        buffer.api.points_in_polygons_device(ps._h, buffer._h, C.c_void_p(ids.ptr or None))
        return ids.to_numpy()


def polygon_mask(buffer: _Buffer, polygons, outside: bool = False, device_mask_ptr: Optional[int] = None):
    """(mask, count): mask[i] = 1 iff point i is in a polygon of the set -- with `outside` iff it is in none, which keeps the points that are
    not finite -- and the number of ones.  mask is a numpy uint8 array, or None when the len(buffer) bytes went to DEVICE memory at
    device_mask_ptr: what filter takes as (ptr, 'device')."""
    from .layout import PointAttributeDataType as T
    count = C.c_uint64()
    with _SetFor(polygons, buffer.api) as ps:
        if device_mask_ptr is not None:
            buffer.api.polygon_mask_device(ps._h, buffer._h, int(bool(outside)), C.c_void_p(int(device_mask_ptr) or None), C.byref(count))
            return None, count.value
        mask = _DeviceArray(buffer.api, T.U8, buffer.len())
        buffer.api.polygon_mask_device(ps._h, buffer._h, int(bool(outside)), C.c_void_p(mask.ptr or None), C.byref(count))
        return mask.to_numpy(), count.value


def crop(buffer: _Buffer, polygons, outside: bool = False, out_buffer_type=None):
    """PDAL's filters.crop with a polygon / lidR's clip_roi: (the points inside the set -- outside it with `outside` -- in buffer order with
    all their attributes, their number).  Mask and compaction stay in device memory.  `buffer` is columnar (filter is defined on
    HashMapBuffer)."""
    with _SetFor(polygons, buffer.api) as ps:
        return _filter_by_device_mask(buffer, out_buffer_type, lambda p: polygon_mask(buffer, ps, outside, device_mask_ptr=p or 1)[1])


def overlay(buffer: _Buffer, attribute: PointAttributeDefinition, polygons, values) -> int:
    """PDAL's filters.overlay / lidR's merge_spatial: the U8 `attribute` of every point inside a polygon becomes values[id], id the point's
    polygon; the other points keep theirs, and so does a point whose polygon has no value (id >= len(values)).  In place, on the device.
    Returns the number of points written."""
    from .layout import PointAttributeDataType as T
    values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1)
    n, written = buffer.len(), C.c_uint64()
    with _SetFor(polygons, buffer.api) as ps:
        ids, vals = _DeviceArray(buffer.api, T.U32, n), _DeviceArray(buffer.api, T.U8, len(values))
        if len(values):
            vals.buffer.set_attribute_range(vals.attribute, range(0, len(values)), values)
        buffer.api.points_in_polygons_device(ps._h, buffer._h, C.c_void_p(ids.ptr or None))
        buffer.api.buffer_set_u8_from_ids_device(buffer._h, attribute.name().encode(), C.c_void_p(ids.ptr or None), C.c_void_p(vals.ptr or None), len(values), C.byref(written))
    return written.value


def crop_kernel_shape(api=None) -> dict:
    """The seams of the point-in-polygon kernels: points per workgroup of the flat and of the banded kernel, and the most entries the flat
    kernel takes (also where the automatic choice changes over: what the LDS holds; the flat kernel was the faster one at every measured
    count up to it)."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).crop_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("flat_points_per_block", "banded_points_per_block", "flat_max_edges"), (x.value for x in v)))


# ---- individual trees: tops by a local-maximum filter, crowns after Silva et al. 2016 (include/pasture_amd.h) ----------------------------------

NO_TREE = 0xFFFFFFFF


@dataclass(frozen=True)
class TreeTops:
    """What tree_tops returns: `indices` (uint32) = the buffer indices of the tops in tree-number order -- by descending height, ties by
    ascending index --, `heights` (float64) their heights, `n_candidates` the valid points at or above min_height, `n_tops` = len(indices);
    `mask` (uint8, one byte per point) is 1 at the tops."""
    indices: np.ndarray
    heights: np.ndarray
    n_candidates: int
    n_tops: int
    mask: np.ndarray


@dataclass(frozen=True)
class TreeSegmentation:
    """What segment_trees returns: `tree_id` (uint32 per point, NO_TREE = 0xFFFFFFFF without a tree; None when the labels went to device
    memory), `counts` (uint32, counts[t] = points labelled t), `n_trees`, `n_labelled` = counts.sum()."""
    tree_id: Optional[np.ndarray]
    counts: np.ndarray
    n_trees: int
    n_labelled: int


def _window_radii(window):
    """window in DIAMETERS, as lidR's ws: a number (fixed), or (a, b, min, max) for a + b*h clamped -> the four radii of the C ABI"""
    if isinstance(window, (int, float, np.integer, np.floating)):
        r = 0.5 * float(window)
        return (r, 0.0, r, r)
    a, b, lo, hi = (float(v) for v in window)
    return (0.5 * a, 0.5 * b, 0.5 * lo, 0.5 * hi)


def tree_tops_device(buffer: _Buffer, window_radii, min_height: float, device_top_mask_ptr: int, device_heights_ptr: int = 0, device_mask_ptr: int = 0,
                     cell_edge: float = 0.0, device_top_indices_ptr: int = 0, capacity: int = 0) -> dict:
    """pst_tree_tops_device: lidR's locate_trees(lmf()) on the device.  window_radii = (a, b, r_min, r_max), RADII: r = min(max(a + b*h,
    r_min), r_max).  A valid point (x, y, h finite, mask byte not zero) with h >= min_height is a top iff no other such point within r of
    it in the XY plane is higher (equal heights: has the lower index).  h = z, or the float64 DEVICE column at device_heights_ptr.  Writes
    len(buffer) bytes at device_top_mask_ptr and, with device_top_indices_ptr and enough capacity, the tops' indices (uint32) in tree order:
    tallest first.  Returns {"n_candidates", "n_tops", "origin", "cell_edge", "dim"}; the last three describe the grid that was used, which
    the result does not depend on."""
    nc, nt, me, dim = C.c_uint64(), C.c_uint64(), (C.c_double * 3)(), (C.c_uint32 * 2)()
    w = (C.c_double * 4)(*[float(v) for v in window_radii])
    buffer.api.tree_tops_device(buffer._h, C.c_void_p(int(device_heights_ptr) or None), C.c_void_p(int(device_mask_ptr) or None), min_height, w, cell_edge,
                                C.c_void_p(int(device_top_mask_ptr) or None), C.c_void_p(int(device_top_indices_ptr) or None), capacity, C.byref(nc), C.byref(nt), me, dim)
    return {"n_candidates": nc.value, "n_tops": nt.value, "origin": (me[0], me[1]), "cell_edge": me[2], "dim": (dim[0], dim[1])}


def tree_tops(buffer: _Buffer, window=(3.0, 0.0, 3.0, 3.0), min_height: float = 2.0, heights=None, mask=None, cell_edge: float = 0.0) -> TreeTops:
    """lidR's locate_trees(lmf(ws = window, hmin = min_height)).  `window` is a DIAMETER, as lidR's ws (window = 2*r): a number for a fixed
    window, or (a, b, min, max) for a + b*h clamped to [min, max].  heights: None for z, a numpy float64 array (uploaded) or the address of a
    float64 DEVICE column -- the heights above ground, as a rule.  mask: None, a numpy uint8 array or a DEVICE address."""
    from .layout import PointAttributeDataType as T
    api, n = buffer.api, buffer.len()
    hptr, hheld = _device_input(api, heights, T.F64, np.float64, n, "heights")
    mptr, mheld = _device_input(api, mask, T.U8, np.uint8, n, "mask")
    top = _DeviceArray(api, T.U8, n)
    radii = _window_radii(window)
    info = tree_tops_device(buffer, radii, min_height, top.ptr or 1, hptr, mptr, cell_edge)
    nt = info["n_tops"]
    idx = _DeviceArray(api, T.U32, nt)
    if nt:
        tree_tops_device(buffer, radii, min_height, top.ptr, hptr, mptr, cell_edge, idx.ptr, nt)
    indices = idx.to_numpy().astype(np.uint32) if nt else np.zeros(0, dtype=np.uint32)
    if heights is None:
        from .layout import attributes as A
        hs = buffer.view_attribute(A.POSITION_3D)[indices.astype(np.int64), 2] if nt else np.zeros(0)
    elif hheld is not None:
        hs = hheld.to_numpy()[indices.astype(np.int64)]
    else:  # a caller's device column: gathered through a one-attribute buffer over it
        hs = _read_device_f64(api, hptr, n)[indices.astype(np.int64)] if nt else np.zeros(0)
    del mheld
    return TreeTops(indices, np.asarray(hs, dtype=np.float64), info["n_candidates"], nt, top.to_numpy().astype(np.uint8) if n else np.zeros(0, dtype=np.uint8))


def _read_device_f64(api, ptr: int, count: int) -> np.ndarray:
    """`count` float64 values at a caller's DEVICE address, copied to the host"""
    from .buffers import ExternalColumnsBuffer
    from .layout import PointAttributeDataType as T, PointLayout
    attribute = PointAttributeDefinition.custom("Values", T.F64)
    view = ExternalColumnsBuffer([ptr], PointLayout.from_attributes([attribute], api=api), count)
    return view.view_attribute(attribute)


def segment_trees_device(buffer: _Buffer, device_top_mask_ptr: int, device_tree_id_ptr: int, max_crown_factor: float = 0.6, exclusion: float = 0.3,
                         min_height: float = 2.0, device_heights_ptr: int = 0, device_mask_ptr: int = 0, cell_edge: float = 0.0, device_counts_ptr: int = 0,
                         counts_capacity: int = 0) -> dict:
    """pst_segment_trees_device: lidR's segment_trees(silva2016()) on the device.  The trees are the valid points with a non-zero byte in the
    DEVICE mask at device_top_mask_ptr, numbered by descending height (ties: ascending index).  A valid point with h >= min_height looks up
    its NEAREST top in the XY plane (ties: the top of smaller index) and gets that tree's number iff it lies within
    0.5 * max_crown_factor * H of it and h >= exclusion * H, H the top's height; every other point gets NO_TREE.  Writes len(buffer) uint32
    at device_tree_id_ptr and, with device_counts_ptr and enough capacity, the points per tree (uint32).  Returns {"n_trees", "n_labelled"}."""
    nt, nl = C.c_uint64(), C.c_uint64()
    buffer.api.segment_trees_device(buffer._h, C.c_void_p(int(device_heights_ptr) or None), C.c_void_p(int(device_mask_ptr) or None),
                                    C.c_void_p(int(device_top_mask_ptr) or None), min_height, max_crown_factor, exclusion, cell_edge,
                                    C.c_void_p(int(device_tree_id_ptr) or None), C.c_void_p(int(device_counts_ptr) or None), counts_capacity, C.byref(nt), C.byref(nl))
    return {"n_trees": nt.value, "n_labelled": nl.value}


def segment_trees(buffer: _Buffer, tops, max_crown_factor: float = 0.6, exclusion: float = 0.3, min_height: float = 2.0, heights=None, mask=None,
                  cell_edge: float = 0.0, device_tree_id_ptr: Optional[int] = None) -> TreeSegmentation:
    """lidR's segment_trees(silva2016(max_cr_factor, exclusion)): see segment_trees_device.  tops: a TreeTops, a numpy uint8 mask with one
    byte per point, or the address of such bytes in DEVICE memory.  heights, mask: as tree_tops.  With device_tree_id_ptr the labels stay in
    DEVICE memory there and the result's tree_id is None."""
    from .layout import PointAttributeDataType as T
    api, n = buffer.api, buffer.len()
    hptr, hheld = _device_input(api, heights, T.F64, np.float64, n, "heights")
    mptr, mheld = _device_input(api, mask, T.U8, np.uint8, n, "mask")
    tptr, theld = _device_input(api, tops.mask if isinstance(tops, TreeTops) else tops, T.U8, np.uint8, n, "tops")
    ids = _DeviceArray(api, T.U32, n) if device_tree_id_ptr is None else None
    id_ptr = (ids.ptr or 1) if ids is not None else int(device_tree_id_ptr)
    info = segment_trees_device(buffer, tptr or 1, id_ptr, max_crown_factor, exclusion, min_height, hptr, mptr, cell_edge)
    nt = info["n_trees"]
    counts = _DeviceArray(api, T.U32, nt)
    if nt:
        info = segment_trees_device(buffer, tptr, id_ptr, max_crown_factor, exclusion, min_height, hptr, mptr, cell_edge, counts.ptr, nt)
    del hheld, mheld, theld
    tree_id = None if ids is None else (ids.to_numpy().astype(np.uint32) if n else np.zeros(0, dtype=np.uint32))
    return TreeSegmentation(tree_id, counts.to_numpy().astype(np.uint32) if nt else np.zeros(0, dtype=np.uint32), nt, info["n_labelled"])


def extract_tree(buffer: _Buffer, segmentation_or_ptr, first: int = 0, count: int = 1, out_buffer_type=None):
    """The points of trees first .. first + count - 1 (tree 0 is the tallest) in buffer order with all their attributes: a TreeSegmentation
    (its labels are uploaded) or the address of len(buffer) uint32 labels in DEVICE memory, through cluster_mask and filter.  `buffer` is
    columnar (filter is defined on HashMapBuffer)."""
    from .layout import PointAttributeDataType as T
    labels = segmentation_or_ptr.tree_id if isinstance(segmentation_or_ptr, TreeSegmentation) else segmentation_or_ptr
    if labels is None:
        raise ValueError("this TreeSegmentation left its labels in device memory: pass their address")
    ptr, held = _device_input(buffer.api, labels, T.U32, np.uint32, buffer.len(), "tree ids")
    out = _filter_by_device_mask(buffer, out_buffer_type, lambda p: cluster_mask(ptr, buffer.len(), first, count, p, api=buffer.api))[0]
    del held
    return out


def trees_kernel_shape(api=None) -> dict:
    """The seams of the tree kernels: candidates per workgroup of the near pass of the filter (one lane each), survivors per workgroup of its
    far pass (one wave each), queries per workgroup of the crown search, points per block partial of the member pass."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(4)]
    (api or product_api()).trees_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "survivors_per_block", "queries_per_block", "bounds_points_per_block"), (x.value for x in v)))


def trees_phase_times(api=None):
    """(candidate index, local-maximum filter, numbering, top index + crown search) in milliseconds of this thread's last tree_tops* or
    segment_trees* call; zeros unless PST_TREES_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "trees_phase_times", 4)


def trees_work(api=None) -> dict:
    """Of this thread's last tree_tops* call: the candidates, those the near pass left to the far pass, and the candidates the far pass
    tested (counted only with PST_TREES_WORK=1 in the environment, else 0)."""
    from ._capi import product_api
    out = (C.c_uint64 * 3)()
    (api or product_api()).trees_work(out)
    return dict(zip(("candidates", "survivors", "far_tested"), (int(x) for x in out)))


# ---- segment statistics: per-label count, box, centroid, covariance and value statistics (include/pasture_amd.h) ------------------------------

# statistic name -> (bit of `stats`, planes); the planes come in ascending bit order
SEGMENT_STATS = {"count": (1, 1), "bounds": (2, 6), "centroid": (4, 3), "covariance": (8, 6), "value_min": (16, 1), "value_max": (32, 1), "value_mean": (64, 1),
                 "value_variance": (128, 1)}
NO_APEX = 0xFFFFFFFF


def segment_stats_bits(stats) -> int:
    """the `stats` word of pst_segment_statistics for a name or an iterable of names of SEGMENT_STATS"""
    names = [stats] if isinstance(stats, str) else list(stats)
    unknown = [s for s in names if s not in SEGMENT_STATS]
    if unknown:
        raise ValueError(f"unknown statistics {unknown}: choose from {list(SEGMENT_STATS)}")
    bits = 0
    for s in names:
        bits |= SEGMENT_STATS[s][0]
    return bits


def segment_planes(bits: int) -> int:
    """the number of float64 planes of n_segments entries pst_segment_statistics writes for this `stats` word"""
    return sum(planes for bit, planes in SEGMENT_STATS.values() if bits & bit)


@dataclass(frozen=True)
class SegmentTable:
    """What segment_statistics returns, one row per segment; a statistic that was not asked for (and every array, when the planes went to
    device memory) is None.  count (float64 [S]); min, max, centroid ([S][3]); covariance ([S][3][3], symmetric); value_min, value_max,
    value_mean, value_variance ([S]); apex (uint32 [S], NO_APEX for a segment without members); n_members = count.sum().  A segment
    without members has count 0 and NaN everywhere else."""
    n_segments: int
    n_members: int
    count: Optional[np.ndarray] = None
    min: Optional[np.ndarray] = None
    max: Optional[np.ndarray] = None
    centroid: Optional[np.ndarray] = None
    covariance: Optional[np.ndarray] = None
    value_min: Optional[np.ndarray] = None
    value_max: Optional[np.ndarray] = None
    value_mean: Optional[np.ndarray] = None
    value_variance: Optional[np.ndarray] = None
    apex: Optional[np.ndarray] = None

    def principal_axes(self):
        """(eigenvalues [S][3] ascending, eigenvectors [S][3][3] with the axes in the columns) of the covariance, by numpy.linalg.eigh on
        the HOST: not part of the bit-exact contract of the table.  NaN for a segment without members."""
        if self.covariance is None:
            raise ValueError("principal_axes needs the 'covariance' statistic")
        values, vectors = np.full((self.n_segments, 3), np.nan), np.full((self.n_segments, 3, 3), np.nan)
        ok = np.isfinite(self.covariance).all(axis=(1, 2))
        if ok.any():
            values[ok], vectors[ok] = np.linalg.eigh(self.covariance[ok])
        return values, vectors


def segment_statistics(buffer: _Buffer, labels, n_segments: int, stats=("count", "bounds", "centroid"), values=None, mask=None, device_out_ptr: Optional[int] = None,
                       device_apex_ptr: Optional[int] = None, return_apex: bool = False) -> SegmentTable:
    """The table of objects behind a segmentation, in one call on the device: per segment s < n_segments the statistics `stats` names
    (SEGMENT_STATS) over the points labelled s.  labels: a numpy integer array with one label per point (uploaded; -1 and 0xFFFFFFFF: no
    segment) or the address of len(buffer) uint32 in DEVICE memory -- what euclidean_clusters, dbscan, region_growing, segment_trees and
    points_in_polygons leave there.  values: None for z, a numpy float64 array or a DEVICE address (the heights above ground); mask: None, a
    numpy uint8 array or a DEVICE address, only points with a non-zero byte take part.  A point with a coordinate or a value that is not
    finite, or a label >= n_segments, belongs to no segment.  device_out_ptr: the planes go to DEVICE memory there, float64
    [segment_planes(bits)][n_segments] in ascending bit order, and the apex (if any) to device_apex_ptr, uint32 [n_segments]; the table's
    arrays are then None.  return_apex: also the apex, per segment the lowest index among its points of the largest value.  Every sum is
    the fixed tree of the header, so the table is the same bytes whatever the storage or the launch shape."""
    from .layout import PointAttributeDataType as T
    bits = segment_stats_bits(stats)
    S = int(n_segments)
    api, n = buffer.api, buffer.len()
    lptr, lheld = _device_input(api, labels, T.U32, np.uint32, n, "labels")
    vptr, vheld = _device_input(api, values, T.F64, np.float64, n, "values")
    mptr, mheld = _device_input(api, mask, T.U8, np.uint8, n, "mask")
    members = C.c_uint64()
    planes = segment_planes(bits)
    if device_out_ptr is not None:
        api.segment_statistics(buffer._h, C.c_void_p(lptr or None), S, C.c_void_p(vptr or None), C.c_void_p(mptr or None), bits, C.c_void_p(int(device_out_ptr) or None),
                               C.c_void_p(int(device_apex_ptr or 0) or None), 0, C.byref(members))
        del lheld, vheld, mheld
        return SegmentTable(S, members.value)
    host = np.full((planes, max(S, 0)), np.nan, dtype=np.float64)
    apex = np.full(max(S, 0), NO_APEX, dtype=np.uint32) if return_apex else None
    api.segment_statistics(buffer._h, C.c_void_p(lptr or None), S, C.c_void_p(vptr or None), C.c_void_p(mptr or None), bits, C.c_void_p(host.ctypes.data if host.size else 1),
                           C.c_void_p(apex.ctypes.data) if apex is not None else None, 1, C.byref(members))
    del lheld, vheld, mheld
    fields, at = {}, 0
    for name, (bit, count) in SEGMENT_STATS.items():
        if bits & bit:
            fields[name] = host[at:at + count]
            at += count
    out = {k: fields[k][0] for k in ("count", "value_min", "value_max", "value_mean", "value_variance") if k in fields}
    if "bounds" in fields:
        out["min"], out["max"] = np.ascontiguousarray(fields["bounds"][:3].T), np.ascontiguousarray(fields["bounds"][3:].T)
    if "centroid" in fields:
        out["centroid"] = np.ascontiguousarray(fields["centroid"].T)
    if "covariance" in fields:
        xx, xy, xz, yy, yz, zz = fields["covariance"]
        out["covariance"] = np.stack([np.stack([xx, xy, xz], axis=1), np.stack([xy, yy, yz], axis=1), np.stack([xz, yz, zz], axis=1)], axis=1)
    return SegmentTable(S, members.value, apex=apex, **out)


def segments_kernel_shape(api=None) -> dict:
    """The seams of the segment kernels: points per workgroup of the key and gather kernels, the group length of the sums (part of the
    definition), groups per workgroup of the fold kernel (one wave each)."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).segments_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "group", "groups_per_block"), (x.value for x in v)))


def segments_phase_times(api=None):
    """(keys + sort + directory, gather, folds + output) in milliseconds of this thread's last segment_statistics call; zeros unless
    PST_SEGMENTS_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "segments_phase_times", 3)


# ---- quantiles: per-cell and per-segment order statistics and counts above a threshold (include/pasture_amd.h) -------------------------------

QUANTILE_METHODS = {"linear": 0, "lower": 1, "higher": 2}


def _quantile_request(probs, above, method):
    """(probs, n, method word, thresholds, n) as the two quantile calls take them; a probability outside [0, 1] and a NaN are the library's to refuse"""
    if method not in QUANTILE_METHODS:
        raise ValueError(f"unknown method {method!r}: choose from {list(QUANTILE_METHODS)}")
    p = [float(x) for x in ([probs] if isinstance(probs, (int, float)) else probs)]
    t = [float(x) for x in ([above] if isinstance(above, (int, float)) else above)]
    return (C.c_double * max(len(p), 1))(*p), len(p), QUANTILE_METHODS[method], (C.c_double * max(len(t), 1))(*t), len(t)


def rasterize_quantiles(buffer: _Buffer, cell_size: float, probs=(0.5,), above=(), method: str = "linear", values=None, device_mask_ptr: Optional[int] = None,
                        origin=None, dim=None, device_out_ptr: Optional[int] = None) -> Raster:
    """Per-cell quantiles and counts above a threshold on rasterize's grid, on the device.  probs: probabilities in [0, 1]; above: thresholds
    (a value counts when it is greater, compared as doubles); method: "linear" (numpy's, R's and lidR's default), "lower" or "higher".
    values, device_mask_ptr, origin and dim: what rasterize takes.  Raster.planes holds "count" (rows, cols), "quantiles" (P, rows, cols) in
    the order of probs and "above" (T, rows, cols) in the order of above; an empty cell has count 0, NaN quantiles and 0 above.
    device_out_ptr: float64 [1 + P + T][rows][cols] goes to DEVICE memory there and Raster.planes is empty.  The result does not depend on
    the order of the points.  (Host planes on the automatic grid cost one pmf_grid call first, to size the arrays.)"""
    c_probs, P, word, c_thr, Tn = _quantile_request(probs, above, method)
    if (origin is None) != (dim is None):
        raise ValueError("origin and dim must be given together or not at all")
    held = None
    if isinstance(values, PointAttributeDefinition):
        held = _values_column(buffer, values)
        values_ptr = held.ptr
    else:
        values_ptr = int(values) if values is not None else 0
    c_origin = (C.c_double * 2)(*origin) if origin is not None else None
    c_dim = (C.c_uint32 * 2)(*dim) if dim is not None else None
    origin_out, dim_out, members = (C.c_double * 2)(), (C.c_uint32 * 2)(), C.c_uint64()
    host = None
    if device_out_ptr is None:
        if dim is not None:
            cols, rows = int(dim[0]), int(dim[1])
        else:
            grid = pmf_grid(buffer, cell_size)
            cols, rows = grid["cols"], grid["rows"]
        host = np.full((1 + P + Tn, rows, cols), np.nan, dtype=np.float64)
        out_ptr, memkind = C.c_void_p(host.ctypes.data if host.size else 1), 1
    else:
        out_ptr, memkind = C.c_void_p(int(device_out_ptr) or None), 0
    buffer.api.rasterize_quantiles(buffer._h, C.c_void_p(values_ptr or None), C.c_void_p(int(device_mask_ptr or 0) or None), cell_size, c_origin, c_dim, c_probs, P, word,
                                   c_thr, Tn, out_ptr, memkind, origin_out, dim_out, C.byref(members))
    del held
    planes = {} if host is None else {"count": host[0], "quantiles": host[1:1 + P], "above": host[1 + P:]}
    return Raster((origin_out[0], origin_out[1]), cell_size, dim_out[0], dim_out[1], members.value, planes)


@dataclass(frozen=True)
class SegmentQuantiles:
    """What segment_quantiles returns: count (float64 [S]), quantiles ([P][S], in the order of probs), above ([T][S], in the order of the
    thresholds) -- each None when the planes went to device memory -- and n_members = count.sum().  A segment without members has count
    0, NaN quantiles and 0 above."""
    n_segments: int
    n_members: int
    count: Optional[np.ndarray] = None
    quantiles: Optional[np.ndarray] = None
    above: Optional[np.ndarray] = None

    def cover(self, t_index: int = 0):
        """above[t_index] / count on the HOST: the share of a segment's values above that threshold (lidR's pzabove2 as a fraction); NaN
        for a segment without members"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.above[t_index] / self.count


def segment_quantiles(buffer: _Buffer, labels, n_segments: int, probs=(0.5,), above=(), method: str = "linear", values=None, mask=None,
                      device_out_ptr: Optional[int] = None) -> SegmentQuantiles:
    """Per-segment quantiles and counts above a threshold, in one call on the device.  labels, values and mask: what segment_statistics takes,
    with its members; probs, above and method: what rasterize_quantiles takes.  device_out_ptr: float64 [1 + P + T][n_segments] goes to
    DEVICE memory there and the arrays are None.  The result does not depend on the order of the points."""
    from .layout import PointAttributeDataType as T
    c_probs, P, word, c_thr, Tn = _quantile_request(probs, above, method)
    S = int(n_segments)
    api, n = buffer.api, buffer.len()
    lptr, lheld = _device_input(api, labels, T.U32, np.uint32, n, "labels")
    vptr, vheld = _device_input(api, values, T.F64, np.float64, n, "values")
    mptr, mheld = _device_input(api, mask, T.U8, np.uint8, n, "mask")
    members = C.c_uint64()
    host = None
    if device_out_ptr is None:
        host = np.full((1 + P + Tn, max(S, 0)), np.nan, dtype=np.float64)
        out_ptr, memkind = C.c_void_p(host.ctypes.data if host.size else 1), 1
    else:
        out_ptr, memkind = C.c_void_p(int(device_out_ptr) or None), 0
    api.segment_quantiles(buffer._h, C.c_void_p(lptr or None), S, C.c_void_p(vptr or None), C.c_void_p(mptr or None), c_probs, P, word, c_thr, Tn, out_ptr, memkind,
                          C.byref(members))
    del lheld, vheld, mheld
    if host is None:
        return SegmentQuantiles(S, members.value)
    return SegmentQuantiles(S, members.value, host[0], host[1:1 + P], host[1 + P:])


def quantiles_kernel_shape(api=None) -> dict:
    """The seams of the quantile kernels: the sorted positions whose groups one workgroup of the LDS kernel owns, the largest group it sorts
    (larger ones take the two radix sorts), and the window of sorted positions it loads and sorts at once."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(3)]
    (api or product_api()).quantiles_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("points_per_block", "cap", "window"), (x.value for x in v)))


def quantiles_phase_times(api=None):
    """(keys + sort + directory, gather, counts + small groups, large groups) in milliseconds of this thread's last rasterize_quantiles or
    segment_quantiles call; zeros unless PST_QUANTILES_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "quantiles_phase_times", 4)


# ---- fixed-radius neighbour search: counts and CSR lists (include/pasture_amd.h) ----------------------------------------------------------------

NO_NEIGHBOUR = 0xFFFFFFFF


@dataclass
class RadiusNeighbours:
    """The neighbour lists of radius_search in CSR form: the list of query i is indices[offsets[i]:offsets[i + 1]] (target buffer indices,
    uint32, nearest first, equal distances by ascending index) with distances (float64, None when they were not asked for) alongside."""
    offsets: np.ndarray
    indices: np.ndarray
    distances: Optional[np.ndarray]

    @property
    def counts(self) -> np.ndarray:
        return np.diff(self.offsets).astype(np.uint32)

    def list(self, i: int):
        """(indices, distances) of query i; distances is None when they were not asked for"""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.indices[a:b], None if self.distances is None else self.distances[a:b]

    def to_padded(self, k: int) -> np.ndarray:
        """uint32 (n, k): each list's k nearest, padded with 0xFFFFFFFF -- what geometric_features(knn=...) takes, so that features can be
        computed over radius neighbourhoods.  A host helper."""
        n = len(self.offsets) - 1
        out = np.full((n, k), NO_NEIGHBOUR, dtype=np.uint32)
        if n == 0 or k == 0 or len(self.indices) == 0:
            return out
        starts = self.offsets[:-1].astype(np.int64)
        take = np.minimum(np.diff(self.offsets.astype(np.int64)), k)
        rows = np.repeat(np.arange(n, dtype=np.int64), take)
        cols = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(take) - take, take)
        out[rows, cols] = self.indices[np.repeat(starts, take) + cols]
        return out


def radius_neighbour_counts(query: _Buffer, target_or_index, radius: float, transform=None, device_counts_ptr: Optional[int] = None):
    """The number of finite targets within `radius` of every point of `query` (sent through `transform` first, if given), the point itself
    included when it is a target: a uint32 (n,) numpy array -- or, with device_counts_ptr (n x uint32 in DEVICE memory), written there, and
    the total is returned.  target_or_index: a buffer, or a NearestNeighbourIndex built over it once and searched many times."""
    from .layout import PointAttributeDataType as T
    total = C.c_uint64()
    counts = None if device_counts_ptr is not None else _DeviceArray(query.api, T.U32, query.len())
    ptr = int(device_counts_ptr) if device_counts_ptr is not None else counts.ptr
    with _IndexFor(target_or_index) as index:
        query.api.radius_neighbour_counts_device(index._h, query._h, _transform12(transform), radius, C.c_void_p(ptr or None), C.byref(total))
    return total.value if counts is None else counts.to_numpy()


def radius_search_device(query: _Buffer, index: NearestNeighbourIndex, radius: float, offsets_ptr: int, indices_ptr: int, distances_ptr: int, capacity: int,
                         transform=None) -> int:
    """The neighbour lists in caller-owned DEVICE memory (addresses): offsets uint64 [n + 1] (required), indices uint32 [capacity], distances
    float64 [capacity] (0 = not wanted).  Returns the total number of entries.  indices_ptr = 0 with capacity = 0 is the counting form: the
    offsets are written and nothing is filled.  A total above capacity raises a PastureError (status 3) whose message carries the total,
    with the offsets written and the two arrays untouched."""
    from ._capi import PastureError
    total = C.c_uint64()
    p = lambda a: C.c_void_p(int(a) or None)  # noqa: E731
    try:
        query.api.radius_search_device(index._h, query._h, _transform12(transform), radius, p(offsets_ptr), p(indices_ptr), p(distances_ptr), capacity, C.byref(total))
    except PastureError as e:
        if e.code != 3:
            raise
        raise PastureError(3, f"{e} (total = {total.value})") from None
    return total.value


def radius_search(query: _Buffer, target_or_index, radius: float, transform=None, return_distances: bool = True) -> RadiusNeighbours:
    """All finite targets within `radius` of every point of `query` (PCL's radiusSearch, scipy's query_ball_point) as a RadiusNeighbours.
    The count first -- it checks every argument before anything is allocated --, then the arrays of exactly that size, then the lists."""
    from .layout import PointAttributeDataType as T
    n = query.len()
    total = C.c_uint64()
    with _IndexFor(target_or_index) as index:
        query.api.radius_neighbour_counts_device(index._h, query._h, _transform12(transform), radius, None, C.byref(total))
        offsets = _DeviceArray(query.api, T.U64, n + 1)
        indices = _DeviceArray(query.api, T.U32, total.value)
        distances = _DeviceArray(query.api, T.F64, total.value) if return_distances else None
        # (an empty array has no address: with capacity 0 the call is the counting form, which is all that is left to do)
        radius_search_device(query, index, radius, offsets.ptr, indices.ptr, distances.ptr if distances else 0, total.value if indices.ptr else 0, transform)
    return RadiusNeighbours(offsets.to_numpy(), indices.to_numpy(), distances.to_numpy() if distances else None)


def radius_kernel_shape(api=None) -> dict:
    """The seams of the radius-search kernels: queries one workgroup of the count and fill kernels owns, the longest list the LDS kernel
    orders (longer ones take the radix sorts), the window of entries it loads and sorts at once, and the entry positions whose lists it owns."""
    from ._capi import product_api
    v = [C.c_uint32() for _ in range(4)]
    (api or product_api()).radius_kernel_shape(*[C.byref(x) for x in v])
    return dict(zip(("queries_per_block", "sort_cap", "sort_window", "sort_positions_per_block"), (x.value for x in v)))


def radius_phase_times(api=None):
    """(query keys + sort, count + scan, fill, order) in milliseconds of this thread's last radius_neighbour_counts* or radius_search* call;
    zeros unless PST_RADIUS_TIMES=1 was set when the library first ran one."""
    return _phase_times(api, "radius_phase_times", 4)
