"""DBSCAN (pst_dbscan, pst_dbscan_kernel_shape, pst_dbscan_phase_times) against tests/dbscan_ref.py.

CPU tests pin the restatement on a hand-computed cloud, its two pair finders against each other, its min_points 1 and 2 against the cluster
restatement, and the argument checks answered on the host.  GPU tests compare the HIP path with the restatement: labels, sizes, core mask and
the three counts with np.array_equal, no tolerance anywhere -- the result is a function of the neighbour predicate alone, which numpy evaluates
with the same roundings."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_ref as R
import dbscan_ref as D
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_clusters import _code, _empty_buffer, chain_case, make_buffer, seam_cloud, snake, spacing
from test_outliers import cloud

U64P = C.POINTER(C.c_uint64)
NONE = 0xFFFFFFFF
N_ = NONE
BIG = 2 ** 64 - 1
POINTS_PER_BLOCK = 256  # asserted against pst_dbscan_kernel_shape below: the parametrisations need it at collection time


def gpu_dbscan(hip, pts, eps, min_points, storage="H", device=False, want_core=True):
    """(labels, sizes, core, (clusters, n_core, n_labelled)) through host or device memory"""
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip, kind=HashMapBuffer if storage == "H" else VectorBuffer)
    n = buf.len()
    if not device:
        r = alg.dbscan(buf, eps, min_points)
        assert r.labels.dtype == np.uint32 and r.sizes.dtype == np.uint64 and r.core.dtype == bool and r.labels.shape == r.core.shape == (n,)
        return r.labels, r.sizes, r.core, (len(r.sizes), r.n_core, r.n_labelled)
    import torch
    dl = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    dc = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    r = alg.dbscan(buf, eps, min_points, device_labels_ptr=dl.data_ptr(), device_core_ptr=dc.data_ptr() if want_core else None)
    assert r.labels is None and r.core is None
    core = dc.cpu().numpy()[:n]
    assert want_core or (core == 7).all(), "a null core pointer: nothing is written"
    return dl.cpu().numpy().view(np.uint32)[:n], r.sizes, core.astype(bool) if want_core else None, (len(r.sizes), r.n_core, r.n_labelled)


def assert_same(got, want, what=""):
    gl, gs, gc, counts = got
    wl, ws, wc = want
    assert np.array_equal(gs, ws), f"{what}: sizes {gs[:8]} ({len(gs)}) vs {ws[:8]} ({len(ws)})"
    bad = np.flatnonzero(gl != wl)
    assert bad.size == 0, f"{what}: {bad.size} of {len(wl)} labels differ, first at {bad[:4]}: {gl[bad[:4]]} vs {wl[bad[:4]]}"
    if gc is not None:
        bad = np.flatnonzero(gc != wc)
        assert bad.size == 0, f"{what}: {bad.size} of {len(wc)} core flags differ, first at {bad[:4]}"
    assert counts == (len(ws), int(wc.sum()), int((wl != NONE).sum())), f"{what}: counts {counts}"


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

HAND = np.array([[1, 0, 0], [np.nan, 0, 0], [2.75, 0, 0], [1.875, 0, 0], [0, 0, 0], [0.5, 0, 0], [1.95, 0, 0.3], [0.5, 0.5, 0], [0.5, -0.5, 0],
                 [3.25, 0, 0], [3.75, 0, 0], [3.25, 0.5, 0], [3.25, -0.5, 0], [4.6, 0, 0], [10, 10, 10]], dtype=np.float64)


def test_restatement_on_a_hand_computed_cloud():
    """eps = 1.  Blob A = the cross {0, 4, 5, 7, 8} around (0.5, 0, 0), blob B = the cross {2, 9, 10, 11, 12} around (3.25, 0, 0): every member
    has the five of its cross within 1 (the arms' tips are exactly 1 apart), so at min_points = 5 all ten are core, and the blobs' nearest
    points 0 = (1, 0, 0) and 2 = (2.75, 0, 0) are 1.75 apart: two clusters.
    Point 3 = (1.875, 0, 0) has d2 = 0.765625 to point 0 and to point 2, exactly: a border point (its neighbours are itself, 0, 2 and 6) that
    goes to the smaller index, A.  Point 6 = (1.95, 0, 0.3) has d2 = 0.9925 to point 0 and 0.73 to point 2: the nearer one has the LARGER
    index and wins, B.  Point 13 = (4.6, 0, 0) sees only point 10 (0.85 away): border of B.  Point 14 is far from everything: noise.
    Point 1 is not finite.  B has 5 + 2 members, A 5 + 1: B is cluster 0.
    At min_points = 4 the points 3 and 6 (four neighbours each) are core and bridge the blobs: one cluster of 13.
    At min_points = 6 only 0 and 2 (seven neighbours: the cross, 3 and 6) and 10 (the cross and 13) are core; every other member of a cross is
    within 1 of its blob's core points and stays as a border point, 3 and 6 choose as before: the same labels."""
    for grid in (False, True):
        def run(points, *a):
            labels, sizes, core = D.dbscan(points, *a, grid=grid)
            return labels.tolist(), sizes.tolist(), np.flatnonzero(core).tolist()
        both = [1, N_, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, N_]
        assert run(HAND, 1.0, 5) == (both, [7, 6], [0, 2, 4, 5, 7, 8, 9, 10, 11, 12])
        assert run(HAND, 1.0, 6) == (both, [7, 6], [0, 2, 10])
        assert run(HAND, 1.0, 4) == ([0, N_, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, N_], [13], [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
        assert run(HAND, 1.0, 8) == ([N_] * 15, [], [])
        # the indices of points 0 and 2 exchanged: the equidistant point 3 follows the smaller index to B, the geometry has not changed
        swapped = HAND.copy()
        swapped[[0, 2]] = HAND[[2, 0]]
        assert run(swapped, 1.0, 5) == ([0, N_, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, N_], [8, 5], [0, 2, 4, 5, 7, 8, 9, 10, 11, 12])
        # one double below 1 the arms' tips no longer see each other: they have four neighbours; the centres, 0 and 2 (with 3 and 6) and 10 (with 13) still have five or more
        labels, sizes, core = run(HAND, float(np.nextafter(1.0, 0.0)), 5)
        assert core == [0, 2, 5, 9, 10] and sizes == [7, 6] and labels == both
    assert all(a.shape == (0,) for a in D.dbscan(np.zeros((0, 3)), 1.0, 3))
    labels, sizes, core = D.dbscan(np.full((3, 3), np.nan), 1.0, 1, grid=True)
    assert labels.tolist() == [N_] * 3 and sizes.shape == (0,) and not core.any()


def _cpu_cases():
    cases = [seam_cloud(shape, n) for shape in ("volume", "clustered") for n in (2, 3, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 1)] + [seam_cloud("clustered", 4096)]
    rng = np.random.default_rng(3)
    blobs = np.concatenate([rng.random((2000, 3)) * 0.02, rng.random((2000, 3)) * 0.02 + 1e9])
    return cases + [(snake(1.0)[:4000], 1.0), (HAND, 1.0), (blobs, 1e-3)]


def test_grid_restatement_equals_brute_force():
    for pts, eps in _cpu_cases():
        for e in (eps, 2.0 * eps):
            bi, bj, bd = D.pairs_brute(pts, e)
            gi, gj, gd = D.pairs_grid(pts, e)
            b, g = np.lexsort((bj, bi)), np.lexsort((gj, gi))
            assert np.array_equal(bi[b], gi[g]) and np.array_equal(bj[b], gj[g]) and np.array_equal(bd[b], gd[g]), (len(pts), e)
            finite = np.isfinite(pts).all(axis=1)
            for min_points in (1, 3, 6):  # (the same pairs in another order: the border choice and the numbering do not depend on it)
                for got, want in zip(D.from_pairs(len(pts), finite, gi, gj, gd, min_points), D.from_pairs(len(pts), finite, bi, bj, bd, min_points)):
                    assert np.array_equal(got, want), (len(pts), e, min_points)


def test_min_points_one_and_two_are_the_clusters():
    for pts, eps in _cpu_cases():
        i, j, d2 = D.pairs_grid(pts, 2.0 * eps)
        for min_points in (1, 2):
            labels, sizes, core = D.from_pairs(len(pts), np.isfinite(pts).all(axis=1), i, j, d2, min_points)
            want = R.label(pts, 2.0 * eps, min_size=min_points, grid=False)
            assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[1]), (len(pts), min_points)
            assert np.array_equal(core, labels != NONE), "no border points"


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def test_kernel_shape(hip):
    assert alg.dbscan_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK}
    assert 64 <= POINTS_PER_BLOCK <= 1024 and POINTS_PER_BLOCK % 64 == 0
    hip.dbscan_kernel_shape(None)  # the pointer is optional
    assert alg.dbscan_phase_times(hip) == (0.0, 0.0, 0.0, 0.0)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    counts = (C.c_uint64 * 3)()
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    assert _code(lambda: hip.dbscan(None, 1.0, 1, fake, fake, 1, None, 0, counts)) == 1
    assert _code(lambda: hip.dbscan(buf._h, 1.0, 1, None, fake, 1, None, 0, counts)) == 1
    assert _code(lambda: hip.dbscan(buf._h, 1.0, 1, fake, fake, 1, None, 0, None)) == 1
    assert _code(lambda: hip.dbscan(buf._h, 1.0, 1, fake, fake, 7, None, 0, counts)) == 1  # no such memory kind
    # 1e-160 and 1e200: finite and positive, but the square is subnormal / infinite
    for eps in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-160, 1e200, 5e-324):
        assert _code(lambda: hip.dbscan(buf._h, eps, 1, fake, fake, 1, None, 0, counts)) == 1, eps
    assert _code(lambda: hip.dbscan(buf._h, 1.0, 0, fake, fake, 1, None, 0, counts)) == 1  # min_points == 0
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: hip.dbscan(f32._h, 1.0, 1, fake, None, 1, None, 0, counts)) == 4
    with pytest.raises(PasturePanic):
        hip.dbscan(f32._h, 1.0, 1, fake, None, 1, None, 0, counts)
    assert _code(lambda: hip.dbscan_phase_times(None)) == 1
    with pytest.raises(ValueError):
        alg.dbscan(buf, 1.0, 1, device_core_ptr=8)  # core flags in device memory need the labels there too


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    counts = (C.c_uint64 * 3)()
    labels, core = (C.c_uint32 * 8)(), (C.c_uint8 * 8)()
    for buf in (_empty_buffer(hip), _empty_buffer(hip, kind=VectorBuffer)):
        with pytest.raises(PastureError) as e:
            hip.dbscan(buf._h, 1.0, 3, labels, core, 1, None, 0, counts)
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 1])
@pytest.mark.parametrize("shape", ["volume", "clustered"])
def test_lengths_around_the_seams(hip, shape, n):
    assert alg.dbscan_kernel_shape(hip)["points_per_block"] == POINTS_PER_BLOCK
    pts, eps = seam_cloud(shape, n)
    if n >= POINTS_PER_BLOCK - 1:  # (fewer than a handful of points cannot show all four)
        labels, sizes, core = D.dbscan(pts, eps, 4, grid=False)
        border, noise = (labels != NONE) & ~core, labels == NONE
        assert core.any() and border.any() and noise.any() and len(sizes) > 1, "the case is to have core, border and noise points and two clusters"
    for factor in (0.5, 1.0, 2.0, 1e3):  # sparser, as is, denser, everything in one cell
        for min_points in (1, 2, 4, 9):
            want = D.dbscan(pts, eps * factor, min_points, grid=False)
            got = gpu_dbscan(hip, pts, eps * factor, min_points, storage="H" if n % 2 else "V", device=min_points == 4)
            assert_same(got, want, f"{shape} {n} x{factor} min_points {min_points}")


def _knife(axis, variant):
    """A centre with one point exactly eps = 0.5 away on either side along `axis`: with itself it has exactly min_points = 3 neighbours.
    generic: two more points far below, so that the grid's minimum corner is elsewhere; at_minimum: the lower point IS the minimum corner (its other coordinates are the centre's);
    negative: every coordinate < 0."""
    centre = {"generic": (77.5, 78.25, 79.0), "at_minimum": (0.5, 0.5, 0.5), "negative": (-12.5, -0.75, -99.0)}[variant]
    pts = np.array([centre] * 3, dtype=np.float64)
    pts[1, axis] -= 0.5
    pts[2, axis] += 0.5
    if variant == "generic":
        pts = np.concatenate([pts, [[-7.75, -8.25, -9.0], [-7.75, -8.25, -60.5]]])
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["generic", "at_minimum", "negative"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_core_knife_edge(hip, axis, variant):
    pts = _knife(axis, variant)
    extra = len(pts) - 3
    below = float(np.nextafter(0.5, 0.0))
    want = D.dbscan(pts, 0.5, 3, grid=False)
    assert want[0].tolist() == [0, 0, 0] + [N_] * extra and want[1].tolist() == [3] and want[2].tolist() == [True, False, False] + [False] * extra
    assert_same(gpu_dbscan(hip, pts, 0.5, 3), want, "at eps: the centre is core, its two neighbours are border points")
    want = D.dbscan(pts, below, 3, grid=False)
    assert (want[0] == NONE).all() and not want[2].any()
    assert_same(gpu_dbscan(hip, pts, below, 3), want, "one double below: nobody has a neighbour")
    # the clusters' chains, whose longest links are exactly eps long
    chain, tol, _, tol_below, _ = chain_case(axis, variant)
    for min_points in (2, 3):
        for eps in (tol, tol_below):
            assert_same(gpu_dbscan(hip, chain, eps, min_points), D.dbscan(chain, eps, min_points, grid=False), f"chain at {eps!r} min_points {min_points}")


def _two_lines(gap, a_first):
    """Two lines of five points 0.25 apart along x, A ending at x = 0 and B starting at x = gap, and the point (0.875, 0, 0) between them.  At
    eps = 1 and min_points = 4 every point of a line is core (four points of its line within 0.75) and the point between has three neighbours
    at the most.  a_first: A's points have the lower indices.  Returns (points, index of the point between, indices of A, indices of B)."""
    a = np.array([[-0.25 * k, 0.0, 0.0] for k in range(5)])
    b = np.array([[gap + 0.25 * k, 0.0, 0.0] for k in range(5)])
    p = np.array([[0.875, 0.0, 0.0]])
    pts = np.concatenate([a, b, p] if a_first else [b, a, p])
    first, second = np.arange(5), np.arange(5, 10)
    return pts, 10, (first if a_first else second), (second if a_first else first)


@pytest.mark.gpu
def test_border_rules(hip):
    for a_first in (True, False):
        # B starts at 1.8125: the point between is 0.875 from A and 0.9375 from B.  Two clusters, never one, and it joins A wherever A's indices are
        pts, p, ia, ib = _two_lines(1.8125, a_first)
        want = D.dbscan(pts, 1.0, 4, grid=False)
        assert want[1].tolist() == [6, 5] and not want[2][p] and want[0][p] == want[0][ia[0]] == 0 and (want[0][ib] == 1).all()
        assert_same(gpu_dbscan(hip, pts, 1.0, 4), want, f"nearer, a_first={a_first}")
        # B starts at 1.75: exactly 0.875 from both.  The smaller buffer index wins: the answer flips with the indices, not with the geometry
        pts, p, ia, ib = _two_lines(1.75, a_first)
        want = D.dbscan(pts, 1.0, 4, grid=False)
        winner = ia if a_first else ib
        assert want[1].tolist() == [6, 5] and not want[2][p] and want[0][p] == want[0][winner[0]] == 0
        assert_same(gpu_dbscan(hip, pts, 1.0, 4), want, f"equidistant, a_first={a_first}")
    assert_same(gpu_dbscan(hip, HAND, 1.0, 5), D.dbscan(HAND, 1.0, 5, grid=False), "the hand-computed cloud")
    # a border point b in the middle of cell (5, 5, 5) of a grid that starts at the origin, its only core neighbour q in each of the 26 cells
    # around it in turn: q, q2, q3 at 0.55, 1.05 and 1.6 times the cell offset from b (q3 is more than 1 from q on every ray); at min_points = 3
    # q and q2 are core, b (which sees q alone) and q3 are border points
    b = np.array([5.5, 5.5, 5.5])
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                d = np.array([dx, dy, dz], dtype=np.float64)
                if not d.any():
                    continue
                pts = np.array([b, b + 0.55 * d, b + 1.05 * d, b + 1.6 * d, [0.0, 0.0, 0.0], [11.0, 11.0, 11.0]])
                want = D.dbscan(pts, 1.0, 3, grid=False)
                assert want[0].tolist() == [0, 0, 0, 0, N_, N_] and want[2].tolist() == [False, True, True, False, False, False], (dx, dy, dz)
                assert_same(gpu_dbscan(hip, pts, 1.0, 3), want, f"core neighbour in cell {(dx, dy, dz)}")


@pytest.mark.gpu
def test_dense_cell(hip):
    """One cell that holds far more points than a workgroup: 5000 coincident points and 100 within a twentieth of eps of them.  Every point is
    within eps of every other: all have 5100 neighbours."""
    rng = np.random.default_rng(12)
    eps = 0.25
    blob = np.concatenate([np.full((5000, 3), 3.0), 3.0 + (rng.random((100, 3)) - 0.5) * (eps / 10.0)])
    blob = blob[rng.permutation(len(blob))]
    labels, sizes, core, counts = gpu_dbscan(hip, blob, eps, 5100)
    assert sizes.tolist() == [5100] and not labels.any() and core.all() and counts == (1, 5100, 5100)
    for min_points in (5101, 2 ** 40):
        labels, sizes, core, counts = gpu_dbscan(hip, blob, eps, min_points, device=min_points == 5101)
        assert sizes.shape == (0,) and (labels == NONE).all() and not core.any() and counts == (0, 0, 0), min_points


@pytest.mark.gpu
def test_deep_component(hip):
    """A single chain of 2^16 links in random index order: every point but the two ends has three neighbours, itself included."""
    eps = 0.37
    rng = np.random.default_rng(13)
    whole = snake(eps)
    assert len(whole) == 1 << 16
    perm = rng.permutation(len(whole))
    pts = whole[perm]
    labels, sizes, core, counts = gpu_dbscan(hip, pts, eps, 3)
    ends = np.flatnonzero((perm == 0) | (perm == len(whole) - 1))
    assert sizes.tolist() == [1 << 16] and not labels.any() and counts == (1, (1 << 16) - 2, 1 << 16)
    assert np.array_equal(np.flatnonzero(~core), ends), "the two ends are border points"
    labels, sizes, core, counts = gpu_dbscan(hip, pts, eps, 4)
    assert (labels == NONE).all() and not core.any() and counts == (0, 0, 0)
    cut = np.delete(whole, [1000, 9000, 17000, 23456, 31000, 44444, 60000], axis=0)
    cut = cut[rng.permutation(len(cut))]
    want = D.dbscan(cut, eps, 3, grid=True)
    assert len(want[1]) == 8 and want[1].sum() == len(cut) and (~want[2]).sum() == 16
    assert_same(gpu_dbscan(hip, cut, eps, 3), want, "cut snake")


_BIG = {}


def big_cloud():
    """200 003 points, and eps = twice their spacing: about six neighbours a point in the sparse half of the cloud, far more in the dense one"""
    if not _BIG:
        pts = cloud(200_003, 19, "clustered")
        pts.setflags(write=False)
        _BIG["case"] = (pts, 2.0 * spacing(pts))
    return _BIG["case"]


@pytest.mark.gpu
def test_equivalences_on_200003_points(hip):
    pts, eps = big_cloud()
    buf = make_buffer(hip, pts, "H")
    for min_points in (1, 2):
        got = alg.dbscan(buf, eps, min_points)
        labels, sizes = alg.euclidean_clusters(buf, eps, min_points, BIG)
        assert got.labels.tobytes() == labels.tobytes() and got.sizes.tobytes() == sizes.tobytes(), min_points
        assert np.array_equal(got.core, labels != NONE) and got.n_core == got.n_labelled == int((labels != NONE).sum())
    want = D.dbscan(pts, eps, 6, grid=True)
    border = (want[0] != NONE) & ~want[2]
    assert len(want[1]) > 100 and want[2].sum() > 10000 and border.sum() > 1000 and (want[0] == NONE).sum() > 1000
    got = alg.dbscan(buf, eps, 6)
    assert_same((got.labels, got.sizes, got.core, (len(got.sizes), got.n_core, got.n_labelled)), want, "min_points 6")


@pytest.mark.gpu
def test_non_finite_points(hip):
    pts = cloud(4000, 16, "clustered")
    eps = 1.5 * spacing(pts)
    rng = np.random.default_rng(17)
    bad = rng.choice(4000, 180, replace=False)
    k = 0
    for coord in range(3):
        for value in (np.nan, np.inf, -np.inf):
            pts[bad[k:k + 20], coord] = value
            k += 20
    good = np.isfinite(pts).all(axis=1)
    assert (~good).sum() == 180
    sub = D.dbscan(pts[good], eps, 4, grid=False)  # the finite subset, mapped back
    labels, core = np.full(4000, NONE, dtype=np.uint32), np.zeros(4000, dtype=bool)
    labels[good], core[good] = sub[0], sub[2]
    want = (labels, sub[1], core)
    assert len(sub[1]) > 1 and core.any() and ((labels != NONE) & ~core).any() and (labels[good] == NONE).any()
    for got, ref in zip(want, D.dbscan(pts, eps, 4, grid=False)):
        assert np.array_equal(got, ref), "the restatement on the whole cloud"
    for storage in ("H", "V"):
        assert_same(gpu_dbscan(hip, pts, eps, 4, storage=storage), want, "non-finite")
    # nothing but non-finite points
    for device in (False, True):
        labels, sizes, core, counts = gpu_dbscan(hip, np.full((100, 3), np.nan), 1.0, 1, device=device)
        assert (labels == NONE).all() and sizes.shape == (0,) and not core.any() and counts == (0, 0, 0)


@pytest.mark.gpu
def test_key_width_fallback(hip):
    """extent / eps = 10^12 is far above 2^21 cells: the cell edge is doubled until the keys fit, and the result is still exact."""
    rng = np.random.default_rng(15)
    pts = np.concatenate([rng.random((2000, 3)) * 0.02, rng.random((2000, 3)) * 0.02 + 1e9])
    pts = pts[rng.permutation(len(pts))]
    want = D.dbscan(pts, 1e-3, 3, grid=False)
    assert len(want[1]) > 2 and want[2].any() and ((want[0] != NONE) & ~want[2]).any() and (want[0] == NONE).any()
    assert_same(gpu_dbscan(hip, pts, 1e-3, 3), want, "two blobs 10^9 apart")


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("storage", ["sliceH", "sliceV", "packedV", "packedH", "external"])
def test_storage(hip, storage, device):
    """A slice (the parent's other points must not be seen), interleaved records with Position3D at an odd byte offset, caller's memory; labels
    and core flags to host and to device memory."""
    pts, eps = seam_cloud("clustered", 3 * POINTS_PER_BLOCK + 1)
    assert_same(gpu_dbscan(hip, pts, 2.0 * eps, 4, storage=storage, device=device), D.dbscan(pts, 2.0 * eps, 4, grid=False), storage)


@pytest.mark.gpu
def test_null_core_and_range_error(hip):
    pts, eps = seam_cloud("clustered", 3 * POINTS_PER_BLOCK + 1)
    n = len(pts)
    want = D.dbscan(pts, 2.0 * eps, 4, grid=False)
    count = len(want[1])
    assert count > 2
    # core == NULL, to host and to device memory
    buf = make_buffer(hip, pts, "H")
    out = np.zeros(n, dtype=np.uint32)
    counts = (C.c_uint64 * 3)()
    hip.dbscan(buf._h, 2.0 * eps, 4, out.ctypes.data_as(C.c_void_p), None, 1, None, 0, counts)
    assert np.array_equal(out, want[0]) and tuple(counts) == (count, int(want[2].sum()), int((want[0] != NONE).sum()))
    got = gpu_dbscan(hip, pts, 2.0 * eps, 4, device=True, want_core=False)
    assert_same(got, want, "no core array on the device")
    # one slot too few for the sizes: PST_ERR_RANGE, with the counts set, the labels and the core flags written
    out[:] = 0
    core = np.full(n, 7, dtype=np.uint8)
    sizes = np.zeros(count, dtype=np.uint64)
    counts = (C.c_uint64 * 3)()
    args = (buf._h, 2.0 * eps, 4, out.ctypes.data_as(C.c_void_p), core.ctypes.data_as(C.c_void_p), 1, sizes.ctypes.data_as(U64P))
    assert _code(lambda: hip.dbscan(*args, count - 1, counts)) == 3
    assert tuple(counts) == (count, int(want[2].sum()), int((want[0] != NONE).sum())) and np.array_equal(out, want[0]) and not sizes.any()
    assert np.array_equal(core.astype(bool), want[2])
    hip.dbscan(*args, count, counts)
    assert np.array_equal(sizes, want[1]) and np.array_equal(out, want[0])


@pytest.mark.gpu
def test_determinism(hip):
    pts, eps = big_cloud()
    buf = make_buffer(hip, pts, "V")
    first, second = alg.dbscan(buf, eps, 5), alg.dbscan(buf, eps, 5)
    assert first.labels.tobytes() == second.labels.tobytes() and first.core.tobytes() == second.core.tobytes() and first.sizes.tobytes() == second.sizes.tobytes()
    assert (first.n_core, first.n_labelled) == (second.n_core, second.n_labelled) and len(first.sizes) > 1 and first.n_labelled > first.n_core > 0


@pytest.mark.gpu
def test_extraction(hip):
    pts, eps = seam_cloud("clustered", 3 * POINTS_PER_BLOCK + 1)
    n = len(pts)
    labels, sizes, _ = D.dbscan(pts, 2.0 * eps, 4, grid=False)
    assert len(sizes) > 2 and (labels == NONE).any()
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY], api=hip)
    buf = HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    intensity = (np.arange(n) * 7 % 65521).astype(np.uint16)
    buf.set_attribute_range(A.INTENSITY, range(0, n), intensity)
    for first, count, keep in ((0, 1, labels == 0), (1, 2, (labels == 1) | (labels == 2)), (0, NONE, labels != NONE), (NONE, 1, np.zeros(n, dtype=bool))):
        out, got_sizes = alg.extract_dbscan_clusters(buf, 2.0 * eps, 4, first_cluster=first, cluster_count=count)
        assert np.array_equal(got_sizes, sizes) and out.len() == int(keep.sum()), (first, count)
        assert np.array_equal(out.view_attribute(A.POSITION_3D), pts[keep]) and np.array_equal(out.view_attribute(A.INTENSITY), intensity[keep])


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/dbscan_objects.py: DBSCAN keeps the five planted objects apart and calls the stray returns noise; Euclidean clusters at the
    same radius join the two largest boxes through the thread and make a cluster of every stray return."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dbscan_objects", os.path.join(root, "examples", "dbscan_objects.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.main(60000)
    assert sorted(k for held in r["dbscan_objects"] for k in held) == [0, 1, 2, 3, 4] and all(len(held) <= 1 for held in r["dbscan_objects"])
    assert r["noise"] >= mod.STRAYS // 2 and r["kept"] == r["labelled"]
    assert sorted(r["euclidean_objects"][0]) == [0, 1] and r["euclidean_singles"] >= mod.STRAYS // 2
