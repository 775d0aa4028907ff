"""Euclidean cluster extraction (pst_euclidean_clusters, pst_cluster_mask_device, pst_cluster_kernel_shape) against tests/cluster_ref.py.

CPU tests pin the restatement on a hand-computed cloud, its two edge finders against each other, and the argument checks answered on the host.
GPU tests compare the HIP path with the restatement: labels and sizes with np.array_equal, no tolerance anywhere -- the result is a function of
the adjacency predicate alone, which numpy evaluates with the same roundings."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import cloud, make_buffer

U64P = C.POINTER(C.c_uint64)
NONE = 0xFFFFFFFF
POINTS_PER_BLOCK = 256  # asserted against pst_cluster_kernel_shape below: the parametrisations need them at collection time
TILE_POINTS = 0         # the traversal kernel stages no candidates in LDS: there is no tile seam


def spacing(pts):
    """About the mean nearest-neighbour distance of a uniform cloud of this many points in this bounding box (0.554 * (V / n)^(1/3)): connecting
    at that radius gives a mean degree of 0.7, far below the percolation threshold -- many clusters of mixed size."""
    pts = np.asarray(pts).reshape(-1, 3)
    if len(pts) < 2:
        return 1.0
    ext = np.maximum(pts.max(axis=0) - pts.min(axis=0), 1e-3)
    return 0.554 * float(np.prod(ext) / len(pts)) ** (1.0 / 3.0)


def gpu_label(hip, pts, tolerance, min_size=1, max_size=2 ** 64 - 1, storage="H", device=False):
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip, kind=HashMapBuffer if storage == "H" else VectorBuffer)
    if not device:
        labels, sizes = alg.euclidean_clusters(buf, tolerance, min_size, max_size)
        assert labels.dtype == np.uint32 and sizes.dtype == np.uint64 and labels.shape == (buf.len(),)
        return labels, sizes
    import torch
    d = torch.full((max(buf.len(), 1),), 7, dtype=torch.int32, device="cuda")
    none, sizes = alg.euclidean_clusters(buf, tolerance, min_size, max_size, device_labels_ptr=d.data_ptr())
    assert none is None
    return d.cpu().numpy().view(np.uint32)[:buf.len()], sizes


def assert_same(got, want, what=""):
    (gl, gs), (wl, ws) = got, want
    assert np.array_equal(gs, ws), f"{what}: sizes {gs[:8]} ({len(gs)}) vs {ws[:8]} ({len(ws)})"
    bad = np.flatnonzero(gl != wl)
    assert bad.size == 0, f"{what}: {bad.size} of {len(wl)} labels differ, first at {bad[:4]}: {gl[bad[:4]]} vs {wl[bad[:4]]}"


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

HAND = np.array([[2.5, 0, 0], [0, 0, 0], [10, 10, 10], [1, 0, 0], [np.nan, 0, 0], [3.5, 0, 0], [0, 1, 0], [1, 1, 0], [10, 11, 10], [-20, 0, 0]], dtype=np.float64)
N_ = NONE


def test_restatement_on_a_hand_computed_cloud():
    """A = the unit square {1, 3, 6, 7}; B = {0, 5}, a unit apart and a gap of 1.5 from A's edge (point 3 to point 0; the diagonal from point 7
    is sqrt(3.25)); a pair {2, 8} a unit apart, far away; the stray point 9; the NaN point 4.
    At tolerance 1.5 the gap closes (2.25 <= 2.25): A + B has 6 points.  One ulp below it does not: A (4), then B and the pair tie at 2 -- B has
    the smaller smallest member (0 < 2) -- then the stray point."""
    for plain in (False, True):
        comp = R.components_brute(HAND, 1.5, plain=plain)
        assert np.array_equal(comp, [0, 0, 2, 0, -1, 0, 0, 0, 2, 9])
        comp = R.components_brute(HAND, np.nextafter(1.5, 0.0), plain=plain)
        assert np.array_equal(comp, [0, 1, 2, 1, -1, 0, 1, 1, 2, 9])
    below = np.nextafter(1.5, 0.0)
    for grid in (False, True):
        def lab(*a):
            labels, sizes = R.label(HAND, *a, grid=grid)
            return labels.tolist(), sizes.tolist()
        assert lab(1.5) == ([0, 0, 1, 0, N_, 0, 0, 0, 1, 2], [6, 2, 1])
        assert lab(below) == ([1, 0, 2, 0, N_, 1, 0, 0, 2, 3], [4, 2, 2, 1])
        # the size filters: points of dropped clusters are in none, the rest is renumbered
        assert lab(1.5, 2) == ([0, 0, 1, 0, N_, 0, 0, 0, 1, N_], [6, 2])
        assert lab(1.5, 1, 5) == ([N_, N_, 0, N_, N_, N_, N_, N_, 0, 1], [2, 1])
        assert lab(below, 1, 2) == ([0, N_, 1, N_, N_, 0, N_, N_, 1, 2], [2, 2, 1])
        assert lab(below, 2, 2) == ([0, N_, 1, N_, N_, 0, N_, N_, 1, N_], [2, 2])
        assert lab(below, 5) == ([N_] * 10, [])
        # nothing is adjacent: every finite point is a cluster of its own, numbered by index
        assert lab(0.5) == ([0, 1, 2, 3, N_, 4, 5, 6, 7, 8], [1] * 9)
        assert lab(1.0) == ([1, 0, 2, 0, N_, 1, 0, 0, 2, 3], [4, 2, 2, 1]) and lab(np.nextafter(1.0, 0.0)) == lab(0.5)
    assert R.label(np.zeros((0, 3)), 1.0)[0].shape == (0,) and R.label(np.zeros((0, 3)), 1.0)[1].shape == (0,)
    assert R.label(np.full((3, 3), np.nan), 1.0, grid=True)[0].tolist() == [N_] * 3


def snake(tolerance, length=31, rows=32, layers=64):
    """A chain of 2^16 points at spacing 0.9 x tolerance that fills a box: rows of `length` points two spacings apart, joined at alternating ends
    by one point half way, layers of such rows joined the same way.  Points that are not consecutive are at least sqrt(2) spacings apart."""
    pts = []
    ix = iy = iz = 0
    dx = dy = 1
    for _ in range(layers):
        for r in range(rows):
            for i in range(length):
                pts.append((ix, iy, iz))
                if i < length - 1:
                    ix += dx
            dx = -dx
            if r < rows - 1:
                pts.append((ix, iy + dy, iz))
                iy += 2 * dy
        dy = -dy
        pts.append((ix, iy, iz + 1))
        iz += 2
    return np.array(pts, dtype=np.float64) * (0.9 * tolerance)


def chain(axis, variant):
    """3000 points along one axis, min + cumsum of a step that is not representable (0.1), shuffled.  generic: two more points far below the
    chain, so that the cloud's minimum is not on it; at_minimum: the chain starts at the cloud's minimum corner; negative: every coordinate < 0."""
    rng = np.random.default_rng(100 + axis)
    start = {"generic": 1000.3, "at_minimum": 0.3, "negative": -5000.7}[variant]
    pts = np.empty((3000, 3))
    pts[:] = {"generic": (77.7, 78.1, 79.3), "at_minimum": (0.3, 0.3, 0.3), "negative": (-12.3, -0.7, -99.1)}[variant]
    pts[:, axis] = start + np.cumsum(np.full(3000, 0.1))
    if variant == "generic":
        pts = np.concatenate([pts, [[-7.7, -8.3, -9.1], [-7.7, -8.3, -60.2]]])
    return pts[rng.permutation(len(pts))]


_CHAIN = {}


def chain_case(axis, variant):
    """(points, tolerance at which every link holds, reference there, the double below, reference there): computed once"""
    if (axis, variant) not in _CHAIN:
        pts = chain(axis, variant)
        x = np.sort(pts[:, axis])[-3000:]
        d = x[1:] - x[:-1]
        g2 = float(((d * d + 0.0) + 0.0).max())  # the predicate's own expression for the longest link
        tol = float(np.sqrt(g2))
        while tol * tol < g2:
            tol = float(np.nextafter(tol, np.inf))
        while float(np.nextafter(tol, 0.0)) * float(np.nextafter(tol, 0.0)) >= g2:
            tol = float(np.nextafter(tol, 0.0))
        below = float(np.nextafter(tol, 0.0))
        _CHAIN[(axis, variant)] = (pts, tol, R.label(pts, tol, grid=False), below, R.label(pts, below, grid=False))
    return _CHAIN[(axis, variant)]


def seam_cloud(shape, n):
    pts = cloud(n, 5, shape) if n else np.zeros((0, 3))
    return pts, spacing(pts)


def tie_cloud():
    """Clusters of 5, 3, 3, 3, 1, 1, 7, 3, 2 points (chains at spacing 1 along x, 50 apart in y), in shuffled index order."""
    groups = [5, 3, 3, 3, 1, 1, 7, 3, 2]
    pts = np.array([[float(i), 50.0 * g, 0.0] for g, m in enumerate(groups) for i in range(m)])
    return pts[np.random.default_rng(9).permutation(len(pts))], groups


def test_grid_restatement_equals_brute_force():
    cases = [seam_cloud(shape, n) for shape in ("volume", "clustered") for n in (2, 3, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 1, 4096)]
    cases += [(chain(0, "generic"), 0.1), (chain(2, "negative"), 0.1000000001), (tie_cloud()[0], 1.0), (snake(1.0)[:4000], 1.0), (HAND, 1.5)]
    rng = np.random.default_rng(3)
    blobs = np.concatenate([rng.random((2000, 3)) * 0.02, rng.random((2000, 3)) * 0.02 + 1e9])
    cases.append((blobs, 1e-3))
    for pts, tol in cases:
        for t in (tol, 2.0 * tol):
            brute, grid = R.components_brute(pts, t), R.components_grid(pts, t)
            assert np.array_equal(brute, grid), (len(pts), t)
    pts, tol = seam_cloud("volume", 3 * POINTS_PER_BLOCK + 1)
    assert np.array_equal(R.components_brute(pts, tol), R.components_brute(pts, tol, plain=True))
    assert len(np.unique(R.components_grid(snake(1.0), 1.0))) == 1 and len(snake(1.0)) == 1 << 16


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def test_kernel_shape(hip):
    assert alg.cluster_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK, "tile_points": TILE_POINTS}
    one = C.c_uint32(7)
    hip.cluster_kernel_shape(None, C.byref(one))  # each pointer is optional
    assert one.value == TILE_POINTS
    hip.cluster_kernel_shape(None, None)
    assert alg.cluster_phase_times(hip) == (0.0, 0.0, 0.0)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    nc, nl = C.c_uint64(), C.c_uint64()
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    c, l = C.byref(nc), C.byref(nl)
    big = 2 ** 64 - 1
    assert _code(lambda: hip.euclidean_clusters(None, 1.0, 1, big, fake, 1, None, 0, c, l)) == 1
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 1, big, None, 1, None, 0, c, l)) == 1
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 1, big, fake, 1, None, 0, None, l)) == 1
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 1, big, fake, 1, None, 0, c, None)) == 1
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 1, big, fake, 7, None, 0, c, l)) == 1  # no such memory kind
    # 1e-160 and 1e200: finite and positive, but the square is subnormal / infinite
    for tolerance in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-160, 1e200, 5e-324):
        assert _code(lambda: hip.euclidean_clusters(buf._h, tolerance, 1, big, fake, 1, None, 0, c, l)) == 1, tolerance
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 0, big, fake, 1, None, 0, c, l)) == 1   # min_size == 0
    assert _code(lambda: hip.euclidean_clusters(buf._h, 1.0, 5, 4, fake, 1, None, 0, c, l)) == 1     # min_size > max_size
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: hip.euclidean_clusters(f32._h, 1.0, 1, big, fake, 1, None, 0, c, l)) == 4
    with pytest.raises(PasturePanic):
        hip.euclidean_clusters(f32._h, 1.0, 1, big, fake, 1, None, 0, c, l)
    # the mask: null arrays of a non-empty range; an empty range is answered on the host
    assert _code(lambda: hip.cluster_mask_device(None, 5, 0, 1, fake)) == 1
    assert _code(lambda: hip.cluster_mask_device(fake, 5, 0, 1, None)) == 1
    hip.cluster_mask_device(None, 0, 0, 1, None)
    assert _code(lambda: hip.cluster_phase_times(None)) == 1


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    nc, nl = C.c_uint64(), C.c_uint64()
    labels = (C.c_uint32 * 8)()
    for buf in (_empty_buffer(hip), _empty_buffer(hip, kind=VectorBuffer)):
        with pytest.raises(PastureError) as e:
            hip.euclidean_clusters(buf._h, 1.0, 1, 2 ** 64 - 1, labels, 1, None, 0, C.byref(nc), C.byref(nl))
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)
    with pytest.raises(PastureError) as e:
        hip.cluster_mask_device(C.c_void_p(8), 5, 0, 1, C.c_void_p(8))
    assert e.value.code == 21


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

def _seam_sizes():
    P, t = POINTS_PER_BLOCK, TILE_POINTS
    sizes = {0, 1, 2, 3, P - 1, P, P + 1, 3 * P + 1} | ({t - 1, t, t + 1, 3 * t + 1} if t else set())
    return sorted(sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("n", _seam_sizes())
@pytest.mark.parametrize("shape", ["volume", "clustered"])
def test_lengths_around_the_seams(hip, shape, n):
    pts, tol = seam_cloud(shape, n)
    want = R.label(pts, tol, grid=False)
    if n >= POINTS_PER_BLOCK - 1:  # (fewer than a handful of points cannot show both)
        assert len(want[1]) > 1 and want[1][0] > 1, "the case is to have more than one cluster and one of more than one point"
    assert_same(gpu_label(hip, pts, tol, storage="H" if n % 2 else "V"), want, f"{shape} {n}")
    for factor in (0.5, 2.0, 1e3):  # sparser, denser, everything in one cell and one cluster
        assert_same(gpu_label(hip, pts, tol * factor), R.label(pts, tol * factor, grid=False), f"{shape} {n} x{factor}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["generic", "at_minimum", "negative"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_grid_knife_edge(hip, axis, variant):
    """Links of a chain that are exactly `tolerance` long: a grid whose cell edge equalled the tolerance would put some of them two cells apart."""
    pts, tol, want, below, want_below = chain_case(axis, variant)
    extra = 2 if variant == "generic" else 0
    assert want[1].tolist() == [3000] + [1] * extra, "at the tolerance every link holds"
    assert len(want_below[1]) > 1 + extra and want_below[1].sum() == len(pts), "one double below it the longest links break"
    assert_same(gpu_label(hip, pts, tol), want, "at the tolerance")
    assert_same(gpu_label(hip, pts, below), want_below, "one double below")


@pytest.mark.gpu
def test_dense_cell(hip):
    """One cell that holds far more points than a workgroup: 5000 coincident points and 100 within a tenth of the tolerance, then a second
    such blob three tolerances away.  The expected labels are literals: every point of a blob is within a fifth of the tolerance of every other,
    and the blobs are more than 2.8 tolerances apart."""
    rng = np.random.default_rng(12)
    tol = 0.25
    blob = np.concatenate([np.full((5000, 3), 3.0), 3.0 + (rng.random((100, 3)) - 0.5) * (tol / 10.0)])
    blob = blob[rng.permutation(len(blob))]
    labels, sizes = gpu_label(hip, blob, tol)
    assert sizes.tolist() == [5100] and not labels.any()
    two = np.concatenate([blob, blob[:4000] + np.array([3.0 * tol, 0.0, 0.0])])
    labels, sizes = gpu_label(hip, two, tol, storage="V")
    assert sizes.tolist() == [5100, 4000] and not labels[:5100].any() and (labels[5100:] == 1).all()


@pytest.mark.gpu
def test_deep_component(hip):
    """A single chain of 2^16 links in random index order (path length, CAS retries), then the same chain cut at 7 places."""
    tol = 0.37
    rng = np.random.default_rng(13)
    pts = snake(tol)
    assert len(pts) == 1 << 16
    pts = pts[rng.permutation(len(pts))]
    labels, sizes = gpu_label(hip, pts, tol)
    assert sizes.tolist() == [1 << 16] and not labels.any()
    assert_same((labels, sizes), R.label(pts, tol, grid=True), "snake")
    whole = snake(tol)
    cut = np.delete(whole, [1000, 9000, 17000, 23456, 31000, 44444, 60000], axis=0)
    cut = cut[rng.permutation(len(cut))]
    want = R.label(cut, tol, grid=True)
    assert len(want[1]) == 8 and want[1].sum() == len(cut)
    assert_same(gpu_label(hip, cut, tol), want, "cut snake")


@pytest.mark.gpu
def test_all_singletons(hip):
    tol = 2.0
    g = np.arange(32, dtype=np.float64) * (1.5 * tol)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = pts[np.random.default_rng(14).permutation(len(pts))]
    n = len(pts)
    assert n == 1 << 15
    labels, sizes = gpu_label(hip, pts, tol)
    assert np.array_equal(labels, np.arange(n, dtype=np.uint32)) and np.array_equal(sizes, np.ones(n, dtype=np.uint64))
    # min_size = 2 keeps none
    buf = make_buffer(hip, pts, "H")
    out = np.zeros(n, dtype=np.uint32)
    nc, nl = C.c_uint64(9), C.c_uint64(9)
    hip.euclidean_clusters(buf._h, tol, 2, 2 ** 64 - 1, out.ctypes.data_as(C.c_void_p), 1, None, 0, C.byref(nc), C.byref(nl))
    assert (out == NONE).all() and (nc.value, nl.value) == (0, 0)
    labels, sizes = alg.euclidean_clusters(buf, tol, 2)
    assert (labels == NONE).all() and sizes.shape == (0,)


@pytest.mark.gpu
def test_key_width_fallback(hip):
    """extent / tolerance = 10^12 is far above 2^21 cells: the cell edge is doubled until the keys fit, and the result is still exact."""
    rng = np.random.default_rng(15)
    pts = np.concatenate([rng.random((2000, 3)) * 0.02, rng.random((2000, 3)) * 0.02 + 1e9])
    pts = pts[rng.permutation(len(pts))]
    want = R.label(pts, 1e-3, grid=False)
    assert len(want[1]) > 2 and want[1][0] > 1
    assert_same(gpu_label(hip, pts, 1e-3), want, "two blobs 10^9 apart")


@pytest.mark.gpu
def test_non_finite_points(hip):
    pts = cloud(4000, 16, "volume")
    tol = spacing(pts)
    rng = np.random.default_rng(17)
    bad = rng.choice(4000, 180, replace=False)
    k = 0
    for coord in range(3):
        for value in (np.nan, np.inf, -np.inf):
            pts[bad[k:k + 20], coord] = value
            k += 20
    good = np.isfinite(pts).all(axis=1)
    assert (~good).sum() == 180
    sub_labels, sub_sizes = R.label(pts[good], tol, grid=False)  # the finite subset, mapped back
    want = np.full(4000, NONE, dtype=np.uint32)
    want[good] = sub_labels
    assert len(sub_sizes) > 1 and sub_sizes[0] > 1
    for storage in ("H", "V"):
        buf = make_buffer(hip, pts, storage)
        out = np.zeros(4000, dtype=np.uint32)
        nc, nl = C.c_uint64(), C.c_uint64()
        hip.euclidean_clusters(buf._h, tol, 1, 2 ** 64 - 1, out.ctypes.data_as(C.c_void_p), 1, None, 0, C.byref(nc), C.byref(nl))
        assert np.array_equal(out, want) and nc.value == len(sub_sizes) and nl.value == int(good.sum())
        assert_same(alg.euclidean_clusters(buf, tol), (want, sub_sizes), "non-finite")
    assert_same((want, sub_sizes), R.label(pts, tol, grid=False), "the restatement on the whole cloud")
    # min_size = 2: n_clustered counts the labelled points only
    labels, sizes = gpu_label(hip, pts, tol, 2)
    assert_same((labels, sizes), R.label(pts, tol, 2, grid=False), "min_size 2")
    # nothing but NaN
    for device in (False, True):
        labels, sizes = gpu_label(hip, np.full((100, 3), np.nan), 1.0, device=device)
        assert (labels == NONE).all() and sizes.shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("storage", ["sliceH", "sliceV", "packedV", "packedH", "external"])
def test_storage(hip, storage, device):
    """A slice (the parent's other points must not be seen), interleaved records with Position3D at an odd byte offset, caller's memory; labels
    to host and to device memory."""
    pts, tol = seam_cloud("clustered", 3 * POINTS_PER_BLOCK + 1)
    assert_same(gpu_label(hip, pts, tol, storage=storage, device=device), R.label(pts, tol, grid=False), storage)


@pytest.mark.gpu
def test_size_filters_and_ties(hip):
    pts, groups = tie_cloud()
    n = len(pts)
    want = R.label(pts, 1.0, grid=False)
    assert want[1].tolist() == sorted(groups, reverse=True)
    for lo, hi in ((1, 2 ** 64 - 1), (2, 2 ** 64 - 1), (1, 3), (3, 3), (2, 5), (4, 6), (8, 2 ** 64 - 1), (7, 7), (1, 1)):
        assert_same(gpu_label(hip, pts, 1.0, lo, hi), R.label(pts, 1.0, lo, hi, grid=False), f"sizes {lo} .. {hi}")
    # one slot too few for the sizes: PST_ERR_RANGE, with the counts set and the labels written
    buf = make_buffer(hip, pts, "H")
    out = np.zeros(n, dtype=np.uint32)
    sizes = np.zeros(len(groups), dtype=np.uint64)
    nc, nl = C.c_uint64(), C.c_uint64()
    args = (buf._h, 1.0, 1, 2 ** 64 - 1, out.ctypes.data_as(C.c_void_p), 1, sizes.ctypes.data_as(U64P))
    assert _code(lambda: hip.euclidean_clusters(*args, len(groups) - 1, C.byref(nc), C.byref(nl))) == 3
    assert (nc.value, nl.value) == (len(groups), n) and np.array_equal(out, want[0]) and not sizes.any()
    hip.euclidean_clusters(*args, len(groups), C.byref(nc), C.byref(nl))
    assert np.array_equal(sizes, want[1]) and np.array_equal(out, want[0])


@pytest.mark.gpu
def test_mask_and_extraction(hip):
    import torch
    pts, tol = seam_cloud("clustered", 3 * POINTS_PER_BLOCK + 1)
    n = len(pts)
    want_labels, want_sizes = R.label(pts, tol, grid=False)
    count = len(want_sizes)
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY], api=hip)
    buf = HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    intensity = (np.arange(n) * 7 % 65521).astype(np.uint16)
    buf.set_attribute_range(A.INTENSITY, range(0, n), intensity)
    d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    _, sizes = alg.euclidean_clusters(buf, tol, device_labels_ptr=d_labels.data_ptr())
    labels = d_labels.cpu().numpy().view(np.uint32)
    assert_same((labels, sizes), (want_labels, want_sizes), "two attributes")
    for first, cnt in ((0, 1), (1, 3), (count - 1, 5), (NONE, 1), (0, NONE), (NONE - 1, 2), (5, 0)):
        mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        alg.cluster_mask(d_labels.data_ptr(), n, first, cnt, mask.data_ptr(), api=hip)
        l64 = labels.astype(np.int64)
        want = ((l64 >= first) & (l64 < first + cnt) & (labels != NONE)).astype(np.uint8)
        assert np.array_equal(mask.cpu().numpy(), want), (first, cnt)
    assert (labels == NONE).sum() == 0  # (no filter here: 0xFFFFFFFF is tested through the filtered call below)
    big, sizes2 = alg.extract_clusters(buf, tol, 1, 2 ** 64 - 1)
    assert np.array_equal(sizes2, want_sizes) and big.len() == int(want_sizes[0])
    assert np.array_equal(big.view_attribute(A.POSITION_3D), pts[want_labels == 0])
    assert np.array_equal(big.view_attribute(A.INTENSITY), intensity[want_labels == 0])
    # clusters 1 .. 2 of those with at least two points; the dropped ones carry 0xFFFFFFFF and are never selected
    fl, fs = R.label(pts, tol, 2, grid=False)
    some, sizes3 = alg.extract_clusters(buf, tol, 2, 2 ** 64 - 1, first_cluster=1, cluster_count=2)
    assert np.array_equal(sizes3, fs) and np.array_equal(some.view_attribute(A.INTENSITY), intensity[(fl == 1) | (fl == 2)])
    none, _ = alg.extract_clusters(buf, tol, 2, 2 ** 64 - 1, first_cluster=NONE, cluster_count=1)
    assert none.len() == 0


@pytest.mark.gpu
def test_determinism(hip):
    pts = cloud(1 << 17, 18, "clustered")
    tol = spacing(pts)
    buf = make_buffer(hip, pts, "H")
    first = alg.euclidean_clusters(buf, tol)
    second = alg.euclidean_clusters(buf, tol)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    want = R.label(pts, tol, grid=True)
    assert len(want[1]) > 1 and want[1][0] > 1
    assert_same(first, want, "2^17 clustered")


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/segment_objects.py: the ground goes, the three largest clusters are the three largest objects of the scene."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("segment_objects", os.path.join(root, "examples", "segment_objects.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sizes, found, planted = mod.main(60000)
    assert len(sizes) >= 3 and found == planted
