"""kNN search with distances, statistical and radius outlier masks (pst_knn_search_device, pst_statistical_outlier_mask, pst_radius_outlier_mask)
against tests/outlier_ref.py.

CPU tests pin the restatement on a hand-computed cloud and the argument checks answered on the host.  GPU tests compare the HIP path with the
restatement: distances and mean neighbour distances bit for bit, masks byte for byte; only the two sums of the statistics carry a bound, the one
any summation order of m non-negative terms obeys (m * 2^-52 relative to the correctly rounded sum)."""
import ctypes as C
import math

import numpy as np
import pytest

import outlier_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import ExternalMemoryBuffer, HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

U64P = C.POINTER(C.c_uint64)
POINTS_PER_BLOCK = 64     # asserted against pst_outlier_kernel_shape below: the parametrisations need them at collection time
REDUCE_BLOCK = 256
REDUCE_POINTS = 1024
BRUTE_MAX = 2048          # KnnCall::brute: clouds up to this size are searched all against all, larger ones through the grid


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def cloud(n, seed, shape):
    """The clouds of the kNN parity tests (test_gpu_parity._normals_inputs)."""
    rng = np.random.default_rng(seed)
    if shape == "volume":
        return rng.random((n, 3)) * np.array([1000.0, 1000.0, 100.0])
    if shape == "surface":
        xy = rng.random((n, 2)) * 500.0
        z = 20.0 * np.sin(xy[:, 0] / 40.0) * np.cos(xy[:, 1] / 55.0) + rng.normal(0, 0.05, n)
        return np.column_stack([xy, z])
    if shape == "clustered":
        a = rng.random((n // 2, 3)) * np.array([400.0, 400.0, 400.0])
        b = rng.random((n - n // 2, 3)) * np.array([200.0, 200.0, 200.0]) + np.array([50.0, 100.0, 150.0])
        return np.concatenate([a, b])[rng.permutation(n)]
    raise ValueError(shape)


_REF = {}


def reference(shape, n, seed=5):
    """(points, sampled queries, distances of their 64 nearest): computed once per cloud; any k <= 64 is a prefix of the sorted list.  Every
    query up to 8192 points, 512 sampled ones above."""
    key = (shape, n, seed)
    if key not in _REF:
        pts = cloud(n, seed, shape)
        q = np.arange(n) if n <= 8192 else np.sort(np.random.default_rng(seed + 1).choice(n, 512, replace=False))
        _, dist = R.knn(pts, 64, q)
        for a in (pts, q, dist):
            a.setflags(write=False)
        _REF[key] = (pts, q, dist)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_restatement_on_a_hand_computed_cloud():
    """A 3 x 3 x 1 unit lattice and one point 10 above its centre, mean_k = 2.  Every lattice point has two neighbours at distance 1: dbar = 1.
    The far point's nearest are the centre (10) and an edge midpoint (sqrt(1 + 100)): dbar = (10 + sqrt(101)) / 2 = D.  Nine values 1 and one D:
    mean = (9 + D) / 10, sum of squared deviations = (D - 1)^2 * 9 / 10, stddev = (D - 1) / sqrt(10); with stddev_mult = 1 the threshold lies
    between 1 and D."""
    pts = np.array([[x, y, 0.0] for x in range(3) for y in range(3)] + [[1.0, 1.0, 10.0]])
    idx, dist = R.knn(pts, 3)
    assert np.array_equal(idx[:, 0], np.arange(10)) and np.all(dist[:, 0] == 0.0)
    assert np.array_equal(idx[0], [0, 1, 3]) and np.array_equal(idx[4], [4, 1, 3]) and np.array_equal(idx[9], [9, 4, 1])  # ties: lower index first
    dbar = R.mean_distances(dist, 2)
    D = (10.0 + math.sqrt(101.0)) / 2.0
    assert np.array_equal(dbar, [1.0] * 9 + [D]) and abs(D - 10.024937810560445) < 1e-14
    mean, stddev, threshold, m = R.statistics(dbar, 1.0)
    assert m == 10
    assert abs(mean - 1.9024937810560445) < 1e-15 and abs(mean - (9.0 + D) / 10.0) < 1e-15
    assert abs(stddev - 2.853935922274422) < 1e-14 and abs(stddev - (D - 1.0) / math.sqrt(10.0)) < 1e-14
    assert abs(threshold - 4.756429703330466) < 1e-14
    assert np.array_equal(R.statistical_mask(dbar, threshold), [1] * 9 + [0])
    # radius: two neighbours within 1 everywhere on the lattice, none within 9.99 of the far point; the border is <=
    assert np.array_equal(R.radius_mask(dist, 1.0, 2), [1] * 9 + [0])
    assert np.array_equal(R.radius_mask(dist, np.nextafter(1.0, 0.0), 2), [0] * 10)
    assert np.array_equal(R.radius_mask(dist, 10.0, 1), [1] * 10) and np.array_equal(R.radius_mask(dist, np.nextafter(10.0, 0.0), 1), [1] * 9 + [0])
    # fewer points than slots: padded with -1 at +inf, and nothing has that many neighbours
    idx, dist = R.knn(pts[:3], 5)
    assert np.array_equal(idx[:, 3:], -np.ones((3, 2))) and np.all(np.isposinf(dist[:, 3:])) and not R.radius_mask(dist, 1e9, 4).any()
    # a NaN point: its own distances are NaN, it is the last neighbour of everyone else, its dbar is not finite
    pts2 = pts.copy()
    pts2[9, 2] = np.nan
    idx, dist = R.knn(pts2, 10)
    assert np.all(idx[:9, 9] == 9) and np.all(np.isnan(dist[:9, 9])) and np.all(np.isnan(dist[9]))
    assert R.statistics(R.mean_distances(dist, 2), 1.0) == (1.0, 0.0, 1.0, 9)


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def test_kernel_shape(hip):
    shape = alg.outlier_kernel_shape(hip)
    assert shape == {"points_per_block": POINTS_PER_BLOCK, "reduce_block": REDUCE_BLOCK, "reduce_points_per_block": REDUCE_POINTS}
    one = C.c_uint32()
    hip.outlier_kernel_shape(None, None, C.byref(one))  # each pointer is optional
    assert one.value == REDUCE_POINTS
    hip.outlier_kernel_shape(None, None, None)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    mask, stats, kept = (C.c_uint8 * 8)(), (C.c_double * 4)(), C.c_uint64()
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    k = C.byref(kept)
    # knn_search
    assert _code(lambda: hip.knn_search_device(None, 8, None, fake)) == 1
    assert _code(lambda: hip.knn_search_device(buf._h, 8, None, None)) == 1          # d_dist is required
    assert _code(lambda: hip.knn_search_device(buf._h, 2, None, fake)) == 12         # k < 3
    assert _code(lambda: hip.knn_search_device(buf._h, 65, None, fake)) == 23        # k > 64
    # statistical
    assert _code(lambda: hip.statistical_outlier_mask(None, 8, 1.0, mask, 1, None, stats, k)) == 1
    assert _code(lambda: hip.statistical_outlier_mask(buf._h, 8, 1.0, None, 1, None, stats, k)) == 1
    assert _code(lambda: hip.statistical_outlier_mask(buf._h, 8, 1.0, mask, 1, None, None, k)) == 1
    assert _code(lambda: hip.statistical_outlier_mask(buf._h, 8, 1.0, mask, 1, None, stats, None)) == 1
    assert _code(lambda: hip.statistical_outlier_mask(buf._h, 8, 1.0, mask, 2, None, stats, k)) == 1      # no such memory kind
    for mean_k in (0, 64, 1000):
        assert _code(lambda: hip.statistical_outlier_mask(buf._h, mean_k, 1.0, mask, 1, None, stats, k)) == 1
    assert _code(lambda: hip.statistical_outlier_mask(buf._h, 8, float("nan"), mask, 1, None, stats, k)) == 1
    # radius
    assert _code(lambda: hip.radius_outlier_mask(None, 1.0, 4, mask, 1, k)) == 1
    assert _code(lambda: hip.radius_outlier_mask(buf._h, 1.0, 4, None, 1, k)) == 1
    assert _code(lambda: hip.radius_outlier_mask(buf._h, 1.0, 4, mask, 1, None)) == 1
    assert _code(lambda: hip.radius_outlier_mask(buf._h, 1.0, 4, mask, 7, k)) == 1
    for mn in (0, 64):
        assert _code(lambda: hip.radius_outlier_mask(buf._h, 1.0, mn, mask, 1, k)) == 1
    for radius in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert _code(lambda: hip.radius_outlier_mask(buf._h, radius, 4, mask, 1, k)) == 1
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: hip.knn_search_device(f32._h, 8, None, fake)) == 4
    assert _code(lambda: hip.statistical_outlier_mask(f32._h, 8, 1.0, mask, 1, None, stats, k)) == 4
    assert _code(lambda: hip.radius_outlier_mask(f32._h, 1.0, 4, mask, 1, k)) == 4
    with pytest.raises(PasturePanic):
        hip.knn_search_device(f32._h, 8, None, fake)


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = _empty_buffer(hip)
    mask, stats, kept = (C.c_uint8 * 8)(), (C.c_double * 4)(), C.c_uint64()
    calls = [lambda: hip.knn_search_device(buf._h, 8, None, C.c_void_p(8)),
             lambda: hip.statistical_outlier_mask(buf._h, 8, 1.0, mask, 1, None, stats, C.byref(kept)),
             lambda: hip.radius_outlier_mask(buf._h, 1.0, 4, mask, 1, C.byref(kept))]
    for call in calls:
        with pytest.raises(PastureError) as e:
            call()
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

def make_buffer(hip, pts, storage):
    """`pts` (n, 3) float64 in the named storage.  packed*: an Intensity (u16) first, so the position sits at byte offset 2 of a 26-byte record;
    external: caller's memory, 25-byte records with the position at byte 1."""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    n = pts.shape[0]
    if storage == "external":
        import torch
        layout = PointLayout.from_attributes_packed([A.CLASSIFICATION, A.POSITION_3D], 1, api=hip)
        rec = np.zeros(n, dtype=layout.numpy_record_dtype())
        rec[A.POSITION_3D.name()] = pts
        t = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        return ExternalMemoryBuffer(t, layout)
    if storage.startswith("slice"):
        pad = np.full((7, 3), 1e6)
        whole = make_buffer(hip, np.concatenate([pad, pts, pad]), storage[5:])
        s = whole.slice(range(7, 7 + n))
        s._parent = whole
        return s
    packed = storage.startswith("packed")
    layout = PointLayout.from_attributes_packed([A.INTENSITY, A.POSITION_3D], 1, api=hip) if packed else PointLayout.from_attributes([A.POSITION_3D], api=hip)
    buf = (HashMapBuffer if storage.endswith("H") else VectorBuffer).new_from_layout(layout)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    return buf


def gpu_statistical(buf, mean_k, mult, device=False):
    """(mask, OutlierStatistics, dbar) with the mask through host or device memory"""
    if not device:
        return alg.statistical_outlier_mask(buf, mean_k, mult, return_mean_distances=True)
    import torch
    m = torch.full((buf.len(),), 7, dtype=torch.uint8, device="cuda")
    none, st, dbar = alg.statistical_outlier_mask(buf, mean_k, mult, device_mask_ptr=m.data_ptr(), return_mean_distances=True)
    assert none is None
    return m.cpu().numpy(), st, dbar


def gpu_radius(buf, radius, min_neighbours, device=False):
    if not device:
        return alg.radius_outlier_mask(buf, radius, min_neighbours)
    import torch
    m = torch.full((buf.len(),), 7, dtype=torch.uint8, device="cuda")
    none, kept = alg.radius_outlier_mask(buf, radius, min_neighbours, device_mask_ptr=m.data_ptr())
    assert none is None
    return m.cpu().numpy(), kept


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    rows = len(got)
    bad = np.flatnonzero((bits(got).reshape(rows, -1) != bits(want).reshape(rows, -1)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {rows} rows differ, first {bad[:4]}: {got[bad[:2]]} vs {want[bad[:2]]}"


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "V"])
@pytest.mark.parametrize("k", [3, 8, 16, 33, 64])
@pytest.mark.parametrize("shape,n", [("volume", 40000), ("surface", 40000), ("clustered", 40000), ("volume", BRUTE_MAX), ("surface", BRUTE_MAX + 1)])
def test_distances_bit_for_bit(hip, shape, n, k, storage):
    pts, q, want = reference(shape, n)
    buf = make_buffer(hip, pts, storage)
    idx, dist = alg.knn_search(buf, k)
    assert idx.shape == (n, k) and dist.shape == (n, k) and idx.dtype == np.int64 and dist.dtype == np.float64
    assert_same_bits(dist[q], want[:, :k], "distances")
    # the lists are the ones compute_normals works on
    knn = alg.compute_normals(buf, k, return_knn=True)[2]
    assert np.array_equal(idx, knn)
    # ... and the distances are those of the listed neighbours (all queries, not only the sampled ones)
    d = pts[idx] - pts[:, None, :]
    assert_same_bits(dist, np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), "distance of the listed neighbour")


@pytest.mark.gpu
def test_knn_search_device_pointers_and_padding(hip):
    """The raw entry point: with and without the index array; a cloud of fewer than k points pads with 0xFFFFFFFF at +inf."""
    import torch
    pts = cloud(5, 3, "volume")
    buf = make_buffer(hip, pts, "H")
    k = 8
    knn = torch.full((5, k), 7, dtype=torch.int32, device="cuda")
    d1 = torch.zeros((5, k), dtype=torch.float64, device="cuda")
    d2 = torch.zeros((5, k), dtype=torch.float64, device="cuda")
    alg.knn_search_device(buf, k, d1.data_ptr(), knn.data_ptr())
    alg.knn_search_device(buf, k, d2.data_ptr())
    want_idx, want = R.knn(pts, k)
    assert_same_bits(d1.cpu().numpy(), want, "distances")
    assert_same_bits(d2.cpu().numpy(), want, "distances without the index array")
    assert np.array_equal(knn.cpu().numpy().astype(np.int64), want_idx)  # int32 -1 == 0xFFFFFFFF
    assert np.all(np.isposinf(want[:, 5:]))
    idx, dist = alg.knn_search(buf, k)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(dist), bits(want))
    for bad_k, code in ((2, 12), (65, 23)):
        assert _code(lambda: alg.knn_search(buf, bad_k)) == code
    assert _code(lambda: alg.knn_search(make_buffer(hip, pts[:2], "H"), 3)) == 11
    assert _code(lambda: alg.statistical_outlier_mask(buf, 5, 1.0)) == 11  # fewer than mean_k + 1 points
    assert _code(lambda: alg.statistical_outlier_mask(make_buffer(hip, pts[:2], "H"), 1, 1.0)) == 11


def _dbar_cases():
    cases = []
    for mean_k in (1, 2, 7, 16, 31, 63):
        P = POINTS_PER_BLOCK
        sizes = {max(3, mean_k + 1), P - 1, P, P + 1, 2 * P + 1, 20000} | ({3} if mean_k <= 2 else set())
        cases += [(mean_k, n) for n in sorted(sizes) if n >= mean_k + 1]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("mean_k,n", _dbar_cases())
def test_mean_distances_bit_for_bit(hip, mean_k, n):
    pts, q, dist = reference("surface", n)
    buf = make_buffer(hip, pts, "H" if mean_k % 2 else "V")
    mask, st, dbar = gpu_statistical(buf, mean_k, 1.0)
    assert dbar.shape == (n,)
    assert_same_bits(dbar[q], R.mean_distances(dist, mean_k), "dbar")
    assert np.array_equal(mask, R.statistical_mask(dbar, st.threshold)) and st.kept == int(mask.sum()) and st.count == n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [REDUCE_POINTS - 1, REDUCE_POINTS, REDUCE_POINTS + 1, 3 * REDUCE_POINTS + 5, REDUCE_BLOCK * REDUCE_POINTS + 1])
def test_statistics_against_the_correctly_rounded_sums(hip, n):
    """mean, stddev and threshold within m * 2^-52 relative of the fsum values -- the bound of ANY summation order of m non-negative terms, each
    partial sum rounded once (m - 1 additions of relative error 2^-53 each, to first order, and the division / square root on top: m * 2^-53 <
    m * 2^-52).  The variance's terms are the squared deviations about the DEVICE's own mean, which numpy rounds exactly as the kernel does."""
    pts = cloud(n, 11, "volume")
    buf = make_buffer(hip, pts, "H")
    mult = 1.5
    mask, st, dbar = gpu_statistical(buf, 2, mult)
    f = dbar[np.isfinite(dbar)]
    m = len(f)
    assert st.count == m == n
    tol = m * 2.0 ** -52
    mean = math.fsum(f) / m
    ss = math.fsum((f - st.mean) * (f - st.mean))
    stddev = math.sqrt(ss / (m - 1))
    print(f"n={n}: mean {st.mean!r} vs {mean!r} ({abs(st.mean - mean) / mean:.3g}), stddev {st.stddev!r} vs {stddev!r} ({abs(st.stddev - stddev) / stddev:.3g}), bound {tol:.3g}")
    assert abs(st.mean - mean) <= tol * mean
    assert abs(st.stddev - stddev) <= tol * stddev
    assert abs(st.threshold - (mean + mult * stddev)) <= tol * (mean + mult * stddev)
    assert st.threshold == st.mean + mult * st.stddev  # two rounded operations on the device's own values
    assert np.array_equal(mask, R.statistical_mask(dbar, st.threshold)) and st.kept == int(mask.sum())
    # fixed-shape sums: the same bits again
    mask2, st2, dbar2 = gpu_statistical(buf, 2, mult, device=True)
    assert st2 == st and np.array_equal(bits(dbar2), bits(dbar)) and np.array_equal(mask2, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n", [("surface", 5000), ("clustered", BRUTE_MAX)])
def test_masks_exact(hip, shape, n):
    pts, q, dist = reference(shape, n)
    assert len(q) == n
    buf = make_buffer(hip, pts, "H")
    for mean_k, mult in ((8, 1.0), (16, 0.0), (3, -0.5), (5, float("inf"))):
        mask, st, dbar = gpu_statistical(buf, mean_k, mult)
        assert_same_bits(dbar, R.mean_distances(dist, mean_k), "dbar")
        assert np.array_equal(mask, R.statistical_mask(dbar, st.threshold)) and st.kept == int(mask.sum())
        dmask, dst, _ = gpu_statistical(buf, mean_k, mult, device=True)
        assert np.array_equal(dmask, mask) and dst == st
        assert (mask.sum() == n) if mult == float("inf") else (0 < mask.sum() < n)
    _, gd = alg.knn_search(buf, 9)
    for mn in (1, 4, 8):
        col = np.sort(gd[:, mn])
        radii = [0.0, float(col[0]), float(col[n // 3]), float(np.nextafter(col[n // 3], 0.0)), float(col[-1]), float(np.nextafter(col[-1], 0.0)),
                 float(gd[17, mn]), float(np.nextafter(gd[17, mn], 0.0)), 2.5, 1e9]
        for radius in radii:
            mask, kept = gpu_radius(buf, radius, mn)
            want = R.radius_mask(dist, radius, mn)
            assert np.array_equal(mask, want), (mn, radius, int(mask.sum()), int(want.sum()))
            assert kept == int(want.sum())
        assert gpu_radius(buf, float(col[-1]), mn)[1] == n and gpu_radius(buf, float(np.nextafter(col[-1], 0.0)), mn)[1] < n  # the border is <=
        dmask, dkept = gpu_radius(buf, float(col[n // 3]), mn, device=True)
        hmask, hkept = gpu_radius(buf, float(col[n // 3]), mn)
        assert np.array_equal(dmask, hmask) and dkept == hkept


@pytest.mark.gpu
def test_what_a_user_expects(hip):
    """A surface and 50 stray returns scattered over a hundred times its diameter: both criteria mask every stray point and no surface point, and
    the filtered buffer is the surface."""
    surface = cloud(20000, 21, "surface")
    rng = np.random.default_rng(22)
    diameter = float(np.linalg.norm(surface.max(axis=0) - surface.min(axis=0)))
    stray = surface.mean(axis=0) + (rng.random((50, 3)) - 0.5) * 100.0 * diameter
    pts = np.concatenate([surface, stray])
    order = rng.permutation(len(pts))
    pts, planted = pts[order], order >= 20000
    buf = make_buffer(hip, pts, "H")
    want_min, want_max = tuple(surface.min(axis=0)), tuple(surface.max(axis=0))

    mask, st = alg.statistical_outlier_mask(buf, 8, 1.0)
    assert not mask[planted].any() and mask[~planted].all() and st.kept == 20000 and st.count == 20050
    clean, st2 = alg.remove_statistical_outliers(buf, 8, 1.0)
    assert st2 == st and clean.len() == 20000
    b = alg.calculate_bounds(clean)
    assert b.min() == want_min and b.max() == want_max
    assert np.array_equal(clean.view_attribute(A.POSITION_3D), pts[~planted])

    mask, kept = alg.radius_outlier_mask(buf, 25.0, 8)
    assert not mask[planted].any() and mask[~planted].all() and kept == 20000
    clean, kept = alg.remove_radius_outliers(buf, 25.0, 8, VectorBuffer)
    assert kept == 20000 and clean.len() == 20000 and isinstance(clean, VectorBuffer)
    b = alg.calculate_bounds(clean)
    assert b.min() == want_min and b.max() == want_max


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 3000])
def test_hostile_coincident_points(hip, n):
    """Every plane fit of the search is degenerate; that is no error here.  All distances are 0: mean, stddev and threshold are 0, everything is kept."""
    buf = make_buffer(hip, np.full((n, 3), 12.5), "H")
    idx, dist = alg.knn_search(buf, 8)
    assert not dist.any() and idx.min() >= 0 and idx.max() < n
    mask, st, dbar = gpu_statistical(buf, 7, 1.0)
    assert not dbar.any() and (st.mean, st.stddev, st.threshold, st.count, st.kept) == (0.0, 0.0, 0.0, n, n) and mask.all()
    mask, kept = gpu_radius(buf, 0.0, 7)
    assert mask.all() and kept == n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 4000])
def test_hostile_duplicates(hip, n):
    """More copies of one point than the search has slots: their lists are all ties at distance 0, in whatever order -- dbar only sees the distances."""
    pts = cloud(n, 31, "volume")
    pts[100:200] = pts[100]
    pts[n - 70:] = pts[n - 1]
    buf = make_buffer(hip, pts, "V")
    _, want = R.knn(pts, 64)
    for mean_k in (16, 63):
        mask, st, dbar = gpu_statistical(buf, mean_k, 1.0)
        assert_same_bits(dbar, R.mean_distances(want, mean_k), "dbar")
        assert not dbar[100:200].any() and np.array_equal(mask, R.statistical_mask(dbar, st.threshold))
    mask, kept = gpu_radius(buf, 0.0, 63)
    assert np.array_equal(mask, R.radius_mask(want, 0.0, 63)) and kept == 170
    _, dist = alg.knn_search(buf, 64)
    assert_same_bits(dist, want, "distances")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1500, 6000])
def test_hostile_non_finite_coordinates(hip, n):
    """5 % of the points carry a NaN or an infinite coordinate: they are masked out and do not count; the finite points are not disturbed."""
    pts = cloud(n, 41, "surface")
    rng = np.random.default_rng(42)
    bad = rng.choice(n, n // 20, replace=False)
    pts[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    good = np.isfinite(pts).all(axis=1)
    buf = make_buffer(hip, pts, "H")
    _, want = R.knn(pts, 17)
    want_dbar = R.mean_distances(want, 16)
    mask, st, dbar = gpu_statistical(buf, 16, 2.0)
    assert_same_bits(dbar[good], want_dbar[good], "dbar of the finite points")
    assert not np.isfinite(dbar[~good]).any() and not np.isfinite(want_dbar[~good]).any()
    assert st.count == int(good.sum()) and not mask[~good].any()
    assert np.array_equal(mask, R.statistical_mask(dbar, st.threshold)) and st.kept == int(mask.sum())
    ref = R.statistics(dbar, 2.0)
    assert abs(st.mean - ref[0]) <= st.count * 2.0 ** -52 * ref[0]
    radius = float(np.median(want[good, 8]))
    mask, kept = gpu_radius(buf, radius, 8)
    assert np.array_equal(mask[good], R.radius_mask(want, radius, 8)[good]) and not mask[~good].any() and kept == int(mask.sum())
    _, dist = alg.knn_search(buf, 17)
    assert_same_bits(dist[good], want[good], "distances of the finite points")


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["sliceH", "sliceV", "packedV", "packedH", "external"])
@pytest.mark.parametrize("n", [700, 3000])
def test_hostile_storage(hip, storage, n):
    """A slice (the parent's other points must not be seen) and interleaved records with Position3D at an odd byte offset."""
    pts, q, want = reference("clustered", n, seed=6)
    buf = make_buffer(hip, pts, storage)
    _, dist = alg.knn_search(buf, 16)
    assert_same_bits(dist, want[:, :16], "distances")
    mask, st, dbar = gpu_statistical(buf, 15, 1.0)
    assert_same_bits(dbar, R.mean_distances(want, 15), "dbar")
    assert np.array_equal(mask, R.statistical_mask(dbar, st.threshold))
    radius = float(np.median(want[:, 6]))
    mask, kept = gpu_radius(buf, radius, 6, device=True)
    assert np.array_equal(mask, R.radius_mask(want, radius, 6)) and kept == int(mask.sum())


@pytest.mark.gpu
def test_fewer_points_than_neighbours_asked_for(hip):
    pts = cloud(5, 51, "volume")
    buf = make_buffer(hip, pts, "H")
    for mn in (5, 8, 63):
        mask, kept = gpu_radius(buf, 1e12, mn)
        assert not mask.any() and kept == 0
    mask, kept = gpu_radius(buf, 1e12, 4)
    assert mask.all() and kept == 5


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/remove_outliers.py: both criteria drop every stray return; the statistical one keeps the whole terrain."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("remove_outliers", os.path.join(root, "examples", "remove_outliers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    st, kept_radius, n_clean, strays_kept = mod.main(20000, 40)
    assert st.count == 20040 and st.kept == n_clean == 20000 and strays_kept == 0 and kept_radius <= 20000
