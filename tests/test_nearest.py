"""Nearest neighbours between two clouds and point-to-point ICP (pst_nn_index_*, pst_nearest_neighbours_device, pst_distance_mask_device,
pst_icp_step, pst_icp) against tests/nn_ref.py.

CPU tests pin the restatement on a hand-computed cloud, its ring walk against its brute force, and the argument checks answered on the host.
GPU tests compare the HIP search with the restatement without a tolerance: indices equal, distances bit for bit.  Only the sums of the ICP step
carry a bound, the worst case of any summation order (see test_icp_step_sums), and the rotation the bound measured against numpy's SVD."""
import ctypes as C
import math

import numpy as np
import pytest

import nn_ref as R
from pasture_amd import PastureError
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import cloud, make_buffer

P = 256                  # queries per workgroup of the search; asserted against pst_nn_kernel_shape: the parametrisations need it at collection time
REDUCE_BLOCK = 256
REDUCE_POINTS = 1024
NONE = 0xFFFFFFFF
INF = float("inf")
UTM = np.array([5.0e5, 5.4e6, 100.0])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def rotation(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    x, y, z = a / np.linalg.norm(a)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    k = 1.0 - c
    return np.array([[c + x * x * k, x * y * k - z * s, x * z * k + y * s], [y * x * k + z * s, c + y * y * k, y * z * k - x * s], [z * x * k - y * s, z * y * k + x * s, c + z * z * k]])


def rigid(axis, degrees, translation, about=(0.0, 0.0, 0.0)):
    """3 x 4 [R | t] of the rotation about the point `about`, then the translation"""
    Rm, c = rotation(axis, degrees), np.asarray(about, dtype=np.float64)
    return np.column_stack([Rm, c - Rm @ c + np.asarray(translation, dtype=np.float64)])


def assert_same(got, want, what):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.uint32 and gd.dtype == np.float64 and gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.flatnonzero((gi != wi) | (bits(gd) != bits(wd)))
    assert bad.size == 0, f"{what}: {bad.size} of {len(wi)} queries differ, first {bad[:4]}: idx {gi[bad[:4]]} vs {wi[bad[:4]]}, dist {gd[bad[:4]]} vs {wd[bad[:4]]}"


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

HAND_TARGETS = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 2.0, 0.0], [10.0, 0.0, 0.0], [0.0, 0.0, 5.0], [1.0, 1.0, 3.0],
                         [1.0, 3.0, 4.0], [1.0, 0.0, np.inf]])
HAND_QUERIES = np.array([[1.0, 0.0, 0.0],      # exactly between targets 0 and 1: the tie goes to 0, distance 1
                         [0.0, 0.25, 0.0],     # target 0 at 0.25
                         [13.0, 0.0, 0.0],     # target 5 at exactly 3
                         [-5.0, -5.0, -5.0],   # outside the AABB: target 0 at sqrt(75)
                         [1.0, 1.0, 2.5],      # target 7 at 0.5
                         [np.nan, 1.0, 1.0],   # not finite: no match
                         [1.0, 0.0, 1e300]])   # d2 overflows to +inf: matched only when max_distance is +inf, at distance +inf


def _hand_checks(search):
    idx, dist = search(HAND_QUERIES, HAND_TARGETS, INF)
    assert np.array_equal(idx, [0, 0, 5, 0, 7, NONE, 0])
    assert np.array_equal(dist, [1.0, 0.25, 3.0, math.sqrt(75.0), 0.5, INF, INF])
    # the bound is <=: exactly max_distance away is matched, one ulp below it is not
    idx, dist = search(HAND_QUERIES, HAND_TARGETS, 3.0)
    assert np.array_equal(idx, [0, 0, 5, NONE, 7, NONE, NONE]) and np.array_equal(dist, [1.0, 0.25, 3.0, INF, 0.5, INF, INF])
    idx, dist = search(HAND_QUERIES, HAND_TARGETS, np.nextafter(3.0, 0.0))
    assert np.array_equal(idx, [0, 0, NONE, NONE, 7, NONE, NONE]) and np.array_equal(dist, [1.0, 0.25, INF, INF, 0.5, INF, INF])
    idx, dist = search(HAND_QUERIES, HAND_TARGETS, 1.0)
    assert np.array_equal(idx, [0, 0, NONE, NONE, 7, NONE, NONE])
    idx, dist = search(HAND_QUERIES, HAND_TARGETS, np.nextafter(1.0, 0.0))
    assert np.array_equal(idx, [NONE, 0, NONE, NONE, 7, NONE, NONE])
    # the tie goes to the lower BUFFER index whatever the order of the targets
    swapped = HAND_TARGETS.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert search(HAND_QUERIES[:1], swapped, INF)[0][0] == 0 and search(HAND_QUERIES[1:2], swapped, INF)[0][0] == 1
    # a translation that puts query 0 onto target 4; a quarter turn about z that puts (0, -2, 0) onto target 1
    idx, dist = search(HAND_QUERIES[:1], HAND_TARGETS, INF, [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 0]])
    assert idx[0] == 4 and dist[0] == 0.0
    idx, dist = search([[0.0, -2.0, 0.0]], HAND_TARGETS, INF, [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]])
    assert idx[0] == 1 and dist[0] == 0.0
    # no finite target, no target at all
    for empty in (HAND_TARGETS[[2, 9]], np.zeros((0, 3))):
        idx, dist = search(HAND_QUERIES, empty, INF)
        assert np.all(idx == NONE) and np.all(np.isposinf(dist))


def test_restatement_on_a_hand_computed_cloud():
    _hand_checks(R.nearest)
    for edge in (0.5, 3.0, 100.0):
        _hand_checks(lambda q, t, m, tr=None: R.nearest_grid(q, t, edge, m, tr))


@pytest.mark.parametrize("shape", ["volume", "surface", "clustered"])
def test_ring_walk_equals_brute_force(shape):
    """From "every point its own cell" to "one cell", with and without a bound, queries inside and outside the targets' box."""
    tgt, qry = cloud(150, 21, shape), np.concatenate([cloud(60, 22, shape), cloud(10, 23, shape) * 3.0 - 500.0])
    extent = np.ptp(tgt, axis=0).max()
    for max_distance in (INF, extent / 8):
        want = R.nearest(qry, tgt, max_distance)
        for edge in (extent / 4000, extent / 40, extent / 5, extent, extent * 10):
            got = R.nearest_grid(qry, tgt, edge, max_distance)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), (edge, max_distance)


def test_icp_step_restatement_recovers_a_known_motion():
    """Exact pairs (the source is the target moved back): one step from the identity returns the motion, with rms = the displacement."""
    tgt = cloud(200, 31, "volume")
    move = rigid((1.0, 2.0, -1.0), 0.01, (0.02, -0.01, 0.03), about=tgt.mean(axis=0))
    src = (tgt - move[:, 3]) @ move[:, :3]  # inverse: R^T (p - t)
    step = R.icp_step(src, tgt, np.eye(3, 4), 5.0)
    assert step["m"] == 200 and np.array_equal(step["idx"], np.arange(200))
    assert np.abs(step["T_out"] - move).max() < 1e-9
    assert abs(np.linalg.det(step["dR"]) - 1.0) < 1e-14
    mirrored = R.kabsch(np.diag([3.0, 2.0, -1.0]))
    assert abs(np.linalg.det(mirrored) - 1.0) < 1e-14 and np.allclose(mirrored, np.eye(3))


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64):
    return HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _d(values):
    return (C.c_double * len(values))(*values)


IDENTITY = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def test_kernel_shape(hip):
    assert alg.nn_kernel_shape(hip) == {"queries_per_block": P, "reduce_block": REDUCE_BLOCK, "reduce_points_per_block": REDUCE_POINTS}
    one = C.c_uint32()
    hip.nn_kernel_shape(None, None, C.byref(one))  # each pointer is optional
    assert one.value == REDUCE_POINTS
    hip.nn_kernel_shape(None, None, None)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf, f32 = _empty_buffer(hip), _empty_buffer(hip, T.Vec3f32)
    out = C.c_void_p()
    fake = C.c_void_p(8)   # stands for an index / a device array: never dereferenced, every call below fails before that
    sums, t12, rms, m, it = _d([0.0] * 17), _d([0.0] * 12), C.c_double(), C.c_uint64(), C.c_uint32()
    ident = _d(IDENTITY)
    # index
    assert _code(lambda: hip.nn_index_create(None, 0.0, C.byref(out))) == 1
    assert _code(lambda: hip.nn_index_create(buf._h, 0.0, None)) == 1
    for edge in (-1.0, float("nan"), INF, -INF):
        assert _code(lambda: hip.nn_index_create(buf._h, edge, C.byref(out))) == 1
    assert _code(lambda: hip.nn_index_create(f32._h, 0.0, C.byref(out))) == 4
    assert _code(lambda: hip.nn_index_grid(None, None, None, None, None)) == 1
    hip.nn_index_destroy(None)  # like free()
    # search
    assert _code(lambda: hip.nearest_neighbours_device(None, buf._h, None, 1.0, fake, fake)) == 1
    assert _code(lambda: hip.nearest_neighbours_device(fake, None, None, 1.0, fake, fake)) == 1
    assert _code(lambda: hip.nearest_neighbours_device(fake, buf._h, None, 1.0, None, None)) == 1   # not both
    bad_distances = (float("nan"), 0.0, -0.0, -1.0, -INF, 1e-160, 1e-170)  # (1e-160)^2 is subnormal, (1e-170)^2 is zero
    for md in bad_distances:
        assert _code(lambda: hip.nearest_neighbours_device(fake, buf._h, None, md, fake, fake)) == 1
    for bad in (float("nan"), INF, -INF):
        for at in (0, 5, 11):
            t = list(IDENTITY)
            t[at] = bad
            assert _code(lambda: hip.nearest_neighbours_device(fake, buf._h, _d(t), 1.0, fake, fake)) == 1
            assert _code(lambda: hip.icp_step(fake, buf._h, _d(t), 1.0, sums, t12)) == 1
            assert _code(lambda: hip.icp(fake, buf._h, _d(t), 1.0, 5, 0.0, t12, C.byref(rms), C.byref(m), C.byref(it))) == 1
    assert _code(lambda: hip.nearest_neighbours_device(fake, f32._h, None, 1.0, fake, fake)) == 4
    # mask
    assert _code(lambda: hip.distance_mask_device(None, 4, 1.0, 0, fake)) == 1
    assert _code(lambda: hip.distance_mask_device(fake, 4, 1.0, 0, None)) == 1
    hip.distance_mask_device(None, 0, 1.0, 0, None)  # nothing to do
    # ICP step
    assert _code(lambda: hip.icp_step(None, buf._h, ident, 1.0, sums, t12)) == 1
    assert _code(lambda: hip.icp_step(fake, None, ident, 1.0, sums, t12)) == 1
    assert _code(lambda: hip.icp_step(fake, buf._h, None, 1.0, sums, t12)) == 1
    assert _code(lambda: hip.icp_step(fake, buf._h, ident, 1.0, None, t12)) == 1
    assert _code(lambda: hip.icp_step(fake, buf._h, ident, 1.0, sums, None)) == 1
    for md in bad_distances:
        assert _code(lambda: hip.icp_step(fake, buf._h, ident, md, sums, t12)) == 1
        assert _code(lambda: hip.icp(fake, buf._h, None, md, 5, 0.0, t12, None, None, None)) == 1
    assert _code(lambda: hip.icp_step(fake, f32._h, ident, 1.0, sums, t12)) == 4
    # ICP loop
    assert _code(lambda: hip.icp(None, buf._h, None, 1.0, 5, 0.0, t12, None, None, None)) == 1
    assert _code(lambda: hip.icp(fake, None, None, 1.0, 5, 0.0, t12, None, None, None)) == 1
    assert _code(lambda: hip.icp(fake, buf._h, None, 1.0, 5, 0.0, None, None, None, None)) == 1
    assert _code(lambda: hip.icp(fake, buf._h, None, 1.0, 0, 0.0, t12, None, None, None)) == 1     # max_iterations == 0
    for tol in (-1e-9, float("nan"), -INF):
        assert _code(lambda: hip.icp(fake, buf._h, None, 1.0, 5, tol, t12, None, None, None)) == 1
    assert _code(lambda: hip.icp(fake, f32._h, None, 1.0, 5, 0.0, t12, None, None, None)) == 4
    # the Python layer's own check of a transform's shape
    with pytest.raises(ValueError):
        alg._transform12(np.eye(3))
    with pytest.raises(ValueError):
        alg._transform12(np.diag([1.0, 1.0, 1.0, 2.0]))
    assert list(alg._transform12(np.eye(4))) == IDENTITY and list(alg._transform12(np.eye(3, 4))) == IDENTITY


_NO_DEVICE_SCRIPT = r"""
import ctypes as C
import numpy as np
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.buffers import ExternalMemoryBuffer
from pasture_amd.layout import PointLayout, attributes as A
hip = pa.product_api()
layout = PointLayout.from_attributes([A.POSITION_3D], api=hip)
points = np.arange(30.0).reshape(10, 3)  # ten points in host memory
buf = ExternalMemoryBuffer(points.ctypes.data, layout, nbytes=points.nbytes)
assert buf.len() == 10
fake = C.c_void_p(8)
ident = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
calls = [lambda: alg.NearestNeighbourIndex(buf), lambda: alg.NearestNeighbourIndex(buf, 2.5),
         lambda: hip.nearest_neighbours_device(fake, buf._h, None, 1.0, fake, fake),
         lambda: hip.distance_mask_device(fake, 10, 1.0, 0, fake),
         lambda: hip.icp_step(fake, buf._h, ident, 1.0, (C.c_double * 17)(), (C.c_double * 12)()),
         lambda: hip.icp(fake, buf._h, None, 1.0, 5, 0.0, (C.c_double * 12)(), None, None, None)]
out = []
for call in calls:
    try:
        call()
        out.append((0, ""))
    except pa.PastureError as e:
        out.append((e.code, "no CPU fallback" in str(e)))
print("codes", out)
"""


def test_no_cpu_fallback_without_device(hip):
    """Without a GPU every compute call is PST_ERR_NO_DEVICE, never a CPU path: NearestNeighbourIndex on a NON-EMPTY buffer first of all.  An
    owned buffer cannot hold a point without a device, but caller's host memory can be wrapped as one when the library is told not to ask the
    runtime about the range (PST_EXTERNAL_UNCHECKED, read once per process: hence the child process).  Empty buffers in this process show
    that the device is looked for before the lengths are."""
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PST_EXTERNAL_UNCHECKED="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"codes {[(21, True)] * 6}" in r.stdout, r.stdout
    buf = _empty_buffer(hip)
    fake, sums, t12 = C.c_void_p(8), _d([0.0] * 17), _d([0.0] * 12)
    with pytest.raises(PastureError) as e:
        alg.NearestNeighbourIndex(buf)
    assert e.value.code == 21 and "no CPU fallback" in str(e.value)
    calls = [lambda: hip.nearest_neighbours_device(fake, buf._h, None, 1.0, fake, fake),
             lambda: hip.distance_mask_device(fake, 4, 1.0, 0, fake),
             lambda: hip.icp_step(fake, buf._h, _d(IDENTITY), 1.0, sums, t12),
             lambda: hip.icp(fake, buf._h, None, 1.0, 5, 0.0, t12, None, None, None)]
    for call in calls:
        with pytest.raises(PastureError) as e:
            call()
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

_REF = {}


def reference(key, make):
    """A restatement's result, computed once per key and left unchanged."""
    if key not in _REF:
        _REF[key] = make()
        for a in _REF[key] if isinstance(_REF[key], tuple) else ():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


def pair(shape, nq, nt):
    """(queries, targets) of one of the kNN clouds, two independent draws"""
    return cloud(nq, 11, shape), cloud(nt, 12, shape)


def lattice(n, spacing=1.0):
    g = np.arange(n, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def buffer_of(hip, pts, storage="H"):
    return make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip)


def search(hip, queries, targets, max_distance=INF, transform=None, cell_edge=0.0, storage=("H", "H")):
    qb, tb = buffer_of(hip, queries, storage[0]), buffer_of(hip, targets, storage[1])
    index = alg.NearestNeighbourIndex(tb, cell_edge)
    try:
        return alg.nearest_neighbours(qb, index, max_distance, transform)
    finally:
        index.destroy()


# ------------------------------------------------------------------------------------------------------------------------------ GPU: search

QUERY_LENGTHS = [1, 2, 63, 64, 65, P - 1, P, P + 1, 2 * P + 1, 1000]


@pytest.mark.gpu
def test_kernel_shape_on_the_gpu(hip):
    assert alg.nn_kernel_shape(hip)["queries_per_block"] == P


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 2, 3, 65, 1000, 4099])
@pytest.mark.parametrize("shape", ["volume", "surface", "clustered"])
def test_lengths(hip, shape, nt):
    """Every query length around the wave and the workgroup against every target length, one index per target, unbounded and bounded."""
    queries, targets = pair(shape, max(QUERY_LENGTHS), nt)
    spacing = np.ptp(targets, axis=0).max() / 10 if nt > 1 else 50.0
    tb = make_buffer(hip, targets, "H")
    index = alg.NearestNeighbourIndex(tb)
    grid = index.grid()
    assert grid["n_finite"] == nt and 1 <= grid["occupied_cells"] <= nt and np.array_equal(grid["origin"], targets.min(axis=0))
    for max_distance in (INF, spacing):
        want = reference(("lengths", shape, nt, max_distance), lambda: R.nearest(queries, targets, max_distance))
        for nq in QUERY_LENGTHS:
            got = alg.nearest_neighbours(make_buffer(hip, queries[:nq], "H"), index, max_distance)
            assert_same(got, (want[0][:nq], want[1][:nq]), f"{shape} {nq} x {nt}, max_distance {max_distance}")
    index.destroy()
    index.destroy()  # twice is harmless


STORAGES = ["H", "V", "packedV", "external", "sliceV"]


@pytest.mark.gpu
@pytest.mark.parametrize("target_storage", STORAGES)
@pytest.mark.parametrize("query_storage", STORAGES)
def test_storages(hip, query_storage, target_storage):
    queries, targets = pair("surface", 300, 500)
    want = reference(("storages",), lambda: R.nearest(queries, targets, INF))
    assert_same(search(hip, queries, targets, storage=(query_storage, target_storage)), want, f"{query_storage} against {target_storage}")


@pytest.mark.gpu
def test_query_is_the_target(hip):
    pts = cloud(700, 13, "volume")
    buf = make_buffer(hip, pts, "V")
    idx, dist = alg.nearest_neighbours(buf, buf)
    assert np.array_equal(idx, np.arange(700)) and np.array_equal(bits(dist), bits(np.zeros(700)))
    # duplicated points: the lowest index of every coincident group
    dup = np.concatenate([pts[:300], pts[100:250], pts[:50]])[np.random.default_rng(14).permutation(500)]
    buf = make_buffer(hip, dup, "H")
    idx, dist = alg.nearest_neighbours(buf, buf)
    first = np.array([np.flatnonzero((dup == p).all(axis=1))[0] for p in dup])
    assert np.array_equal(idx, first) and not dist.any()
    assert_same((idx, dist), R.nearest(dup, dup), "duplicates")


@pytest.mark.gpu
@pytest.mark.parametrize("permuted", [False, True])
def test_ties(hip, permuted):
    """Targets on an integer lattice; queries at the centres of its cubes (eight targets at the same distance), of their faces (four) and of
    their edges (two).  Permuted targets: the lowest buffer index is not the first in cell order."""
    targets = lattice(5)
    if permuted:
        targets = targets[np.random.default_rng(15).permutation(len(targets))]
    corners = lattice(4)
    queries = np.concatenate([corners + 0.5, corners + [0.5, 0.5, 0.0], corners + [0.0, 0.5, 0.5], corners + [0.5, 0.0, 0.0], corners + [0.0, 0.0, 0.5]])
    want = R.nearest(queries, targets)
    d2 = R.squared_distances(queries[:, None, :], targets[None, :, :])
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert np.array_equal(np.unique(ties), [2, 4, 8])
    assert np.array_equal(want[0], np.argmax(d2 == d2.min(axis=1, keepdims=True), axis=1))  # the lowest index of the tied ones
    for cell_edge in (0.0, 1.0, 0.4, 3.0):
        assert_same(search(hip, queries, targets, cell_edge=cell_edge), want, f"ties, cell edge {cell_edge}")


@pytest.mark.gpu
def test_knife_edge(hip):
    """Lattice targets 100 apart; queries exactly 13 from their only candidate, along x and along (3, 4, 12) (9 + 16 + 144 = 169 exactly).
    max_distance = 13 matches them, the next double below 13 does not."""
    targets = lattice(4, 100.0)
    queries = np.concatenate([targets + [13.0, 0.0, 0.0], targets - [0.0, 13.0, 0.0], targets + [3.0, 4.0, 12.0], targets - [12.0, 3.0, 4.0], targets + [1.0, 0.0, 0.0]])
    n = len(targets)
    below = np.nextafter(13.0, 0.0)
    for cell_edge in (0.0, 13.0, 100.0, 7.0):
        for max_distance, matched in ((13.0, True), (below, False)):
            want = R.nearest(queries, targets, max_distance)
            assert np.array_equal(want[0][:4 * n] != NONE, np.full(4 * n, matched)) and np.all(want[0][4 * n:] == np.arange(n))
            if matched:
                assert np.array_equal(want[0][:4 * n], np.tile(np.arange(n), 4)) and np.all(want[1][:4 * n] == 13.0)
            assert_same(search(hip, queries, targets, max_distance, cell_edge=cell_edge), want, f"knife edge {max_distance!r}, cell edge {cell_edge}")


def _doubled_edge(edge, extent):
    while max(extent) / edge >= float((1 << 21) - 1):
        edge *= 2.0
    return edge


@pytest.mark.gpu
@pytest.mark.parametrize("stretched", [False, True])
def test_grid_independence(hip, stretched):
    """One pair of 1000-point clouds through indices of very different grids: all give the restatement's bits.  stretched: x times 2^22, so that
    a cell edge of 1 would need more than 2^21 - 1 cells and must be doubled."""
    queries, targets = pair("volume", 1000, 1000)
    if stretched:
        queries, targets = queries * [2.0 ** 22, 1.0, 1.0], targets * [2.0 ** 22, 1.0, 1.0]
    want = reference(("grid", stretched), lambda: R.nearest(queries, targets, INF))
    extent = np.ptp(targets, axis=0)
    spacing = (np.prod(extent) / len(targets)) ** (1.0 / 3.0)
    qb, tb = make_buffer(hip, queries, "H"), make_buffer(hip, targets, "H")
    edges = {"automatic": 0.0, "huge": 10.0 * extent.max(), "tiny": 1.0 if stretched else spacing / 10.0}
    for name, edge in edges.items():
        index = alg.NearestNeighbourIndex(tb, edge)
        grid = index.grid()
        if edge:
            assert grid["cell_edge"] == _doubled_edge(edge, extent), name
            assert grid["dim"] == tuple(int(e / grid["cell_edge"]) + 1 for e in extent)
        else:
            assert 2.0 <= grid["n_finite"] / grid["occupied_cells"] <= 16.0, grid
        if stretched and name == "tiny":
            assert grid["cell_edge"] == 2048.0  # 1000 * 2^22 / 2^11 is the first quotient below 2^21 - 1
        assert max(grid["dim"]) <= (1 << 21) - 1
        assert_same(alg.nearest_neighbours(qb, index), want, f"{name} cell edge, grid {grid}")
        index.destroy()


@pytest.mark.gpu
def test_automatic_edge_on_a_sheet(hip):
    """A sheet fills a small share of its box: the edge guessed from the volume is corrected by the count of occupied cells."""
    targets = cloud(20000, 16, "surface")
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    grid = index.grid()
    assert 2.0 <= grid["n_finite"] / grid["occupied_cells"] <= 16.0, grid
    cells = np.floor((targets - targets.min(axis=0)) / grid["cell_edge"]).astype(np.int64)
    assert grid["occupied_cells"] == len(np.unique(cells, axis=0)) and grid["dim"] == tuple(cells.max(axis=0) + 1)
    index.destroy()


@pytest.mark.gpu
def test_outside_and_empty_regions(hip):
    queries, targets = pair("volume", 200, 1000)
    extent = np.ptp(targets, axis=0).max()
    far = queries * 1e-3 + extent * 1e6 * np.array([[1.0, -1.0, 0.5]])
    assert_same(search(hip, far, targets), R.nearest(far, targets), "10^6 extents away, unbounded")
    got = search(hip, far, targets, max_distance=extent)
    assert np.all(got[0] == NONE) and np.all(np.isposinf(got[1]))
    # outside along one axis only, and just outside: the clamped cell is a face cell
    near = queries + [extent * 1.5, 0.0, 0.0]
    for max_distance in (INF, extent * 0.6):
        assert_same(search(hip, near, targets, max_distance), R.nearest(near, targets, max_distance), "beside the box")
    # two clusters 1000 apart, queries in the empty middle
    rng = np.random.default_rng(17)
    two = np.concatenate([rng.random((400, 3)) * 10.0, rng.random((400, 3)) * 10.0 + [1000.0, 0.0, 0.0]])
    middle = rng.random((300, 3)) * [200.0, 10.0, 10.0] + [400.0, 0.0, 0.0]
    for cell_edge in (0.0, 2.0):
        for max_distance in (INF, 450.0):
            assert_same(search(hip, middle, two, max_distance, cell_edge=cell_edge), R.nearest(middle, two, max_distance), f"middle, cell edge {cell_edge}")
    # a query cloud entirely inside one cell
    inside = targets[7] + rng.random((300, 3)) * 1e-3
    assert_same(search(hip, inside, targets), R.nearest(inside, targets), "one cell")


@pytest.mark.gpu
def test_degenerate_targets(hip):
    queries = cloud(300, 18, "volume")
    rng = np.random.default_rng(19)
    flat = cloud(500, 20, "volume")
    flat[:, 2] = 50.0
    line = np.outer(rng.random(500), [700.0, -300.0, 40.0]) + [100.0, 600.0, 20.0]
    same = np.tile([[500.0, 500.0, 50.0]], (100, 1))
    one = np.full((200, 3), np.nan)
    one[137] = [400.0, 300.0, 20.0]
    one[5, 0], one[9] = np.inf, [1.0, 2.0, -np.inf]
    for name, targets in (("coplanar", flat), ("collinear", line), ("one point", same), ("one finite among NaNs", one)):
        for max_distance in (INF, 100.0):
            assert_same(search(hip, queries, targets, max_distance), R.nearest(queries, targets, max_distance), name)
    tb = make_buffer(hip, flat, "H")
    index = alg.NearestNeighbourIndex(tb)
    assert index.grid()["dim"][2] == 1
    index.destroy()
    for name, targets in (("no finite target", np.full((50, 3), np.nan)), ("no target", np.zeros((0, 3)))):
        index = alg.NearestNeighbourIndex(buffer_of(hip, targets))
        assert index.grid()["n_finite"] == 0 and index.grid()["occupied_cells"] == 0
        idx, dist = alg.nearest_neighbours(make_buffer(hip, queries, "V"), index)
        assert np.all(idx == NONE) and np.all(np.isposinf(dist)), name
        index.destroy()
    # no query
    idx, dist = search(hip, np.zeros((0, 3)), flat)
    assert idx.shape == (0,) and dist.shape == (0,)


@pytest.mark.gpu
def test_non_finite_queries(hip):
    queries, targets = pair("volume", 400, 1000)
    queries = queries.copy()
    bad = []
    for k, value in enumerate((np.nan, np.inf, -np.inf)):
        for axis in range(3):
            at = 3 + 17 * (3 * k + axis)
            queries[at, axis] = value
            bad.append(at)
    want = R.nearest(queries, targets)
    assert np.all(want[0][bad] == NONE) and np.all(np.isposinf(want[1][bad])) and (want[0] != NONE).sum() == 400 - 9
    assert_same(search(hip, queries, targets), want, "non-finite queries")
    assert_same(search(hip, queries, targets, transform=np.eye(3, 4)), R.nearest(queries, targets, INF, np.eye(3, 4)), "non-finite queries through the identity")


@pytest.mark.gpu
def test_transform(hip):
    """About 30 degrees around an oblique axis and a translation of UTM size, against the restatement given the same 12 doubles."""
    queries, targets = pair("surface", 1000, 2000)
    move = rigid((1.0, -2.0, 0.5), 30.0, UTM)
    targets = R.apply_transform(targets, move) + np.random.default_rng(24).normal(0.0, 0.3, (2000, 3))
    for max_distance in (INF, 5.0):
        want = R.nearest(queries, targets, max_distance, move)
        assert (want[0] != NONE).sum() > 100
        assert_same(search(hip, queries, targets, max_distance, transform=move), want, f"transform, max_distance {max_distance}")
    four = np.vstack([move, [0.0, 0.0, 0.0, 1.0]])
    assert_same(search(hip, queries, targets, transform=four), R.nearest(queries, targets, INF, move), "4 x 4")


@pytest.mark.gpu
def test_nullable_outputs(hip):
    import torch
    queries, targets = pair("clustered", 777, 1500)
    want = R.nearest(queries, targets, 30.0)
    qb, index = make_buffer(hip, queries, "H"), alg.NearestNeighbourIndex(make_buffer(hip, targets, "V"))
    idx = [torch.full((777,), 7, dtype=torch.int32, device="cuda") for _ in range(2)]
    dist = [torch.full((777,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    alg.nearest_neighbours_device(qb, index, 30.0, idx_ptr=idx[0].data_ptr(), dist_ptr=dist[0].data_ptr())
    alg.nearest_neighbours_device(qb, index, 30.0, idx_ptr=idx[1].data_ptr())
    alg.nearest_neighbours_device(qb, index, 30.0, dist_ptr=dist[1].data_ptr())
    for i, d in zip(idx, dist):
        assert_same((i.cpu().numpy().view(np.uint32), d.cpu().numpy()), want, "device pointers")
    index.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_distance_mask(hip, n):
    import torch
    threshold = 2.5
    special = [0.0, threshold, np.nextafter(threshold, INF), np.nextafter(threshold, 0.0), INF, np.nan, -0.0, 1e300]
    values = np.resize(np.array(special), n)
    values[len(special):] = np.random.default_rng(25).random(max(0, n - len(special))) * 5.0
    dist = torch.from_numpy(values).cuda()
    with np.errstate(invalid="ignore"):
        near = values <= threshold
    for keep_far in (False, True):
        mask = torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda")
        alg.distance_mask(dist.data_ptr(), n, threshold, keep_far, mask.data_ptr(), api=hip)
        got = mask.cpu().numpy()
        assert got[n] == 7 and np.array_equal(got[:n], (~near if keep_far else near).astype(np.uint8))


_LIMIT_SCRIPT = r"""
import ctypes as C, sys
import numpy as np, torch
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.layout import PointLayout, attributes as A
hip = pa.product_api()
layout = PointLayout.from_attributes([A.POSITION_3D], api=hip)
small = pa.HashMapBuffer.new_from_layout(layout)
small.resize(8)
small.set_attribute_range(A.POSITION_3D, range(0, 8), np.arange(24.0).reshape(8, 3))
index = alg.NearestNeighbourIndex(small)
real = torch.zeros(4096, dtype=torch.uint8, device="cuda")  # where a refused search would have written its indices
host = np.zeros(512)  # HOST memory under the over-long buffers: the device could not even read it
codes = []
for points in (2 ** 32 - 16, 2 ** 32 + 5):
    huge = C.c_void_p()
    hip.buffer_wrap_external(layout._h, C.c_void_p(host.ctypes.data), points * 24, C.byref(huge))
    out, ident = C.c_void_p(), (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    calls = [lambda: hip.nn_index_create(huge, 0.0, C.byref(out)),
             lambda: hip.nearest_neighbours_device(index._h, huge, None, 1.0, C.c_void_p(real.data_ptr()), None),
             lambda: hip.icp_step(index._h, huge, ident, 1.0, (C.c_double * 17)(), (C.c_double * 12)()),
             lambda: hip.icp(index._h, huge, None, 1.0, 3, 0.0, (C.c_double * 12)(), None, None, None)]
    for call in calls:
        try:
            call()
            codes.append(0)
        except pa.PastureError as e:
            codes.append(e.code)
    hip.buffer_destroy(huge)
idx, dist = alg.nearest_neighbours(small, index)
print("codes", codes, "then", idx.tolist(), float(dist.max()))
"""


@pytest.mark.gpu
def test_limits_and_recovery(hip):
    """The length limit by status code.  A cloud of 2^32 - 16 points is 96 GiB of positions, so the buffer is 4 KiB of host memory wrapped
    under that length, in a process of its own that may tell the library not to ask the runtime about the range (PST_EXTERNAL_UNCHECKED is
    read once per process).  Nothing reads the memory: the lengths are refused before anything is launched.  One call after the refused ones works."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PST_EXTERNAL_UNCHECKED="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _LIMIT_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"codes {[23] * 8} then {list(range(8))} 0.0" in r.stdout, r.stdout
    # in this process: a step with nothing in reach is refused, and the next call works
    queries, targets = pair("volume", 100, 300)
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    assert _code(lambda: alg.icp_step(index, make_buffer(hip, queries, "H"), np.eye(3, 4), 1e-6)) == 11  # nothing within a micrometre
    assert_same(alg.nearest_neighbours(make_buffer(hip, queries, "H"), index), R.nearest(queries, targets), "after refused calls")
    index.destroy()


@pytest.mark.gpu
def test_index_outlives_its_target_and_the_scratch_pool(hip):
    queries, targets = pair("surface", 500, 3000)
    tb = make_buffer(hip, targets, "V")
    index = alg.NearestNeighbourIndex(tb)
    tb.resize(10)      # the storage moves
    del tb
    other = make_buffer(hip, cloud(5000, 26, "volume"), "H")  # something else may take the freed memory
    alg.release_scratch(hip)
    assert_same(alg.nearest_neighbours(make_buffer(hip, queries, "H"), index), R.nearest(queries, targets), "after the target has gone")
    del other
    index.destroy()


@pytest.mark.gpu
def test_cloud_to_cloud_and_filter(hip):
    """The distances as a mask for filter: the points of one scan that the other does not have."""
    import torch
    rng = np.random.default_rng(27)
    base = cloud(2000, 28, "surface")
    added = rng.random((100, 3)) * [50.0, 50.0, 5.0] + [200.0, 200.0, 60.0]
    scan_a, scan_b = base, np.concatenate([base + rng.normal(0.0, 0.01, base.shape), added])
    ab, bb = make_buffer(hip, scan_a, "H"), make_buffer(hip, scan_b, "H")
    dist = alg.cloud_to_cloud_distances(bb, ab)
    assert np.array_equal(bits(dist), bits(R.nearest(scan_b, scan_a)[1]))
    d = torch.from_numpy(dist).cuda()
    mask = torch.zeros(len(scan_b), dtype=torch.uint8, device="cuda")
    alg.distance_mask(d.data_ptr(), len(scan_b), 1.0, True, mask.data_ptr(), api=hip)
    changed = bb.filter(HashMapBuffer, (mask.data_ptr(), "device"))
    assert changed.len() == 100 and np.array_equal(changed.view_attribute(A.POSITION_3D), added)


# --------------------------------------------------------------------------------------------------------------------------------- GPU: ICP

def icp_pair(n_source, n_target, seed=41):
    """A terrain-like sheet with relief at UTM-sized coordinates: the targets, and as source another draw of the same surface moved by a small
    rigid motion; T_in is a guess that is close to the motion's inverse but not equal to it."""
    rng = np.random.default_rng(seed)

    def surface(n):
        xy = rng.random((n, 2)) * 200.0
        z = 8.0 * np.sin(xy[:, 0] / 17.0) * np.cos(xy[:, 1] / 23.0) + 0.02 * xy[:, 0] + np.where((xy[:, 0] % 50.0 < 12.0) & (xy[:, 1] % 60.0 < 15.0), 6.0, 0.0)
        return np.column_stack([xy, z]) + UTM
    targets, source = surface(n_target), surface(n_source)
    centre = UTM + [100.0, 100.0, 0.0]
    move = rigid((0.2, -0.1, 1.0), 1.5, (0.8, -0.6, 0.3), about=centre)
    source = (source - move[:, 3]) @ move[:, :3]          # the inverse motion: `move` brings the source back
    guess = rigid((0.1, 0.3, 1.0), 1.2, (0.5, -0.4, 0.2), about=centre)
    return source, targets, guess, move


def _icp_reference(n_source, n_target):
    """(source, targets, T_in, max_distance, idx of all sources): the nearest search is shared by every prefix of the source."""
    def make():
        source, targets, guess, _ = icp_pair(n_source, n_target)
        return source, targets, guess, 4.0, R.nearest(source, targets, 4.0, guess)[0]
    return reference(("icp", n_source, n_target), make)


def _step_reference(n_source, n_target, n):
    def make():
        source, targets, guess, max_distance, idx = _icp_reference(n_source, n_target)
        return (R.icp_step(source[:n], targets, guess, max_distance, idx=idx[:n]),)
    return reference(("icp step", n_source, n_target, n), make)[0]


ICP_CASES = [(1500, 3000, 1500)] + [(REDUCE_POINTS + 1, 3000, n) for n in (REDUCE_POINTS - 1, REDUCE_POINTS, REDUCE_POINTS + 1)] + \
            [(REDUCE_BLOCK * REDUCE_POINTS + 1, 300, n) for n in (REDUCE_BLOCK * REDUCE_POINTS - 1, REDUCE_BLOCK * REDUCE_POINTS, REDUCE_BLOCK * REDUCE_POINTS + 1)]
EPS = 2.0 ** -53


@pytest.mark.gpu
@pytest.mark.parametrize("n_source,n_target,n", ICP_CASES)
def test_icp_step_sums(hip, n_source, n_target, n):
    """m is equal; every sum S (of cq, cp, H and sum_d2) is within 2 * m * 2^-53 * sum|term| of the fsum value: the worst case of any summation
    order of m terms, times two for the terms' own rounding.  cq and cp are not sums but o + S / m, rounded to a double: at UTM size an ulp (9.3e-10 at
    5.4e6) is far above the bound on S / m (about 3e-11 at m = 1500), so a value within the bound of the restatement's may still be a
    different double.  For them the assertion is therefore: within the bound, OR exactly one of the two doubles next to the restatement's
    centroid.  Two calls give identical bits.  (On the MI355X the largest error was 9.0e-4 of the bound for H and 1.2e-5 for sum_d2.)"""
    source, targets, guess, max_distance, _ = _icp_reference(n_source, n_target)
    want = _step_reference(n_source, n_target, n)
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    sb = make_buffer(hip, source[:n], "V")
    sums, t_out = alg.icp_step(index, sb, guess, max_distance)
    again = alg.icp_step(index, sb, guess, max_distance)
    assert np.array_equal(bits(sums), bits(again[0])) and np.array_equal(bits(t_out), bits(again[1]))
    assert np.array_equal(index.grid()["origin"], targets.min(axis=0))
    m = want["m"]
    assert sums[0] == m and m > n // 10
    got = {"cq": sums[1:4], "cp": sums[4:7], "H": sums[7:16].reshape(3, 3), "sum_d2": sums[16]}
    for name, value in got.items():
        bound = 2.0 * m * EPS * np.asarray(want["abs"][name])
        value, ref = np.asarray(value), np.asarray(want[name])
        err = np.abs(value - ref)
        ok = err <= bound
        if name in ("cq", "cp"):
            ok = ok | (value == np.nextafter(ref, np.inf)) | (value == np.nextafter(ref, -np.inf))
            print(f"{name}: {int((err > bound).sum())} entries on a neighbouring double")
        print(f"{name}: largest error / bound = {np.max(err / bound):.3g}")
        assert np.all(ok), f"{name}: {value} vs {ref}, error {err}, bound {bound}"
    index.destroy()


# The largest entry-wise difference measured on the MI355X between the device's step (Horn's quaternion, Jacobi) and numpy's Kabsch of the
# restatement's own H, over ICP_CASES: rotation entries and translation entries (the latter at 5.4e6).  The test asserts 32 times these: the
# two solvers differ, and the sensitivity of dR to H depends on H's singular-value gaps.
MEASURED_ROTATION = 1.22e-15     # the cases gave 2.0e-16 .. 1.22e-15
MEASURED_TRANSLATION = 6.51e-9   # 7.9e-10 .. 6.51e-9


@pytest.mark.gpu
@pytest.mark.parametrize("n_source,n_target,n", ICP_CASES)
def test_icp_step_transform_against_kabsch(hip, n_source, n_target, n):
    source, targets, guess, max_distance, _ = _icp_reference(n_source, n_target)
    want = _step_reference(n_source, n_target, n)
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    sums, t_out = alg.icp_step(index, make_buffer(hip, source[:n], "H"), guess, max_distance)
    index.destroy()
    d_rot = np.abs(t_out[:, :3] - want["T_out"][:, :3]).max()
    d_tra = np.abs(t_out[:, 3] - want["T_out"][:, 3]).max()
    print(f"rotation entries differ by at most {d_rot:.3g}, translation entries by {d_tra:.3g}")
    rot = t_out[:, :3] @ np.linalg.inv(guess[:, :3])
    assert np.abs(rot.T @ rot - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(rot) - 1.0) < 1e-14
    assert d_rot <= 32 * MEASURED_ROTATION and d_tra <= 32 * MEASURED_TRANSLATION


@pytest.mark.gpu
def test_icp_is_the_step_in_a_loop(hip):
    source, targets, guess, move = icp_pair(1500, 3000)
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    sb = make_buffer(hip, source, "H")

    def by_steps(init, max_iterations, tolerance):
        t, last, steps = np.array(init), None, 0
        while steps < max_iterations:
            sums, t = alg.icp_step(index, sb, t, 4.0)
            rms = math.sqrt(sums[16] / sums[0])
            steps += 1
            settled = last is not None and abs(rms - last) <= tolerance
            last = rms
            if settled:
                break
        return t, last, int(sums[0]), steps

    for init, max_iterations, tolerance in ((guess, 4, 0.0), (guess, 50, 1e-3), (np.eye(3, 4), 7, 1e-12), (guess, 1, INF), (guess, 50, INF)):
        want = by_steps(init, max_iterations, tolerance)
        got = alg.icp(sb, index, 4.0, max_iterations, tolerance, init)
        assert np.array_equal(bits(got[0]), bits(want[0])) and bits(got[1]) == bits(want[1]) and got[2:] == want[2:], (max_iterations, tolerance, got, want)
        assert 1 <= got[3] <= max_iterations
    assert alg.icp(sb, index, 4.0, 50, INF, guess)[3] == 2       # any two steps differ by at most +inf
    none = alg.icp(sb, index, 4.0, 3)                             # init None is the identity
    ident = alg.icp(sb, index, 4.0, 3, 0.0, np.eye(3, 4))
    assert np.array_equal(bits(none[0]), bits(ident[0])) and none[1:] == ident[1:]
    by_buffer = alg.icp(sb, make_buffer(hip, targets, "V"), 4.0, 3)  # a buffer in place of an index
    assert np.array_equal(bits(by_buffer[0]), bits(none[0]))
    index.destroy()


@pytest.mark.gpu
def test_icp_recovers_a_rigid_motion(hip):
    """Exact pairs in a volume cloud whose spacing (about 7) is far above the displacement (about 1): the loop converges onto the motion.  The
    coordinates are of UTM size, so a position carries about 1e-9 of rounding: the recovered motion must reproduce the targets to 1e-6."""
    targets = np.random.default_rng(42).random((3000, 3)) * 100.0 + UTM
    move = rigid((1.0, 1.0, 0.3), 0.5, (0.6, -0.5, 0.4), about=UTM + 50.0)
    source = ((targets - move[:, 3]) @ move[:, :3])[::2]
    t, rms, matched, steps = alg.icp(make_buffer(hip, source, "V"), make_buffer(hip, targets, "H"), 5.0, 50, 1e-9)
    assert matched == 1500 and steps < 50 and rms < 1e-6
    assert np.abs(R.apply_transform(source, t) - targets[::2]).max() < 1e-6
    assert np.abs(t[:, :3] - move[:, :3]).max() < 1e-8


@pytest.mark.gpu
def test_icp_degenerate_matches(hip):
    """Fewer than three matches is PST_ERR_TOO_FEW_POINTS; collinear matches (a rank-deficient H) still return a proper rotation."""
    targets = np.outer(np.arange(200.0), [1.0, 2.0, -0.5]) + UTM
    source = targets[20:180:2] + [0.01, -0.02, 0.03]
    index = alg.NearestNeighbourIndex(make_buffer(hip, targets, "H"))
    sums, t = alg.icp_step(index, make_buffer(hip, source, "H"), np.eye(3, 4), 1.0)
    assert sums[0] == 80 and np.all(np.isfinite(t))
    assert np.abs(t[:, :3].T @ t[:, :3] - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(t[:, :3]) - 1.0) < 1e-14
    assert _code(lambda: alg.icp_step(index, make_buffer(hip, source[:2], "H"), np.eye(3, 4), 1.0)) == 11
    assert _code(lambda: alg.icp(make_buffer(hip, source, "H"), index, 1e-3, 5)) == 11
    assert _code(lambda: alg.icp_step(index, buffer_of(hip, np.zeros((0, 3))), np.eye(3, 4), 1.0)) == 11
    index.destroy()
    empty = alg.NearestNeighbourIndex(buffer_of(hip, np.zeros((0, 3))))
    assert _code(lambda: alg.icp_step(empty, make_buffer(hip, source, "H"), np.eye(3, 4), 1.0)) == 11
    empty.destroy()


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/align_scans.py: ICP brings the displaced scan back to within a third of the 0.6 that then separates "new" from "seen" (the
    scans' own spacing is 0.2), and what the keep-far mask and the filter leave in the overlap is the box only the second scan has: at
    least half of its 1293 points (its lowest rows stand within 0.6 of the ground), and nothing outside its footprint."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("align_scans", os.path.join(root, "examples", "align_scans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    residual, found = mod.main()
    print(f"residual {residual:.4f}, {len(found)} points found")
    cx, cy, sx, sy, h = mod.NEW_BOX
    assert residual < 0.2
    assert len(found) >= len(mod.box_points(mod.NEW_BOX)) // 2
    assert np.all(np.abs(found[:, 0] - cx) <= sx / 2 + 0.2) and np.all(np.abs(found[:, 1] - cy) <= sy / 2 + 0.2)
