"""Region growing (pst_region_growing_from_knn, pst_region_growing, pst_region_kernel_shape, pst_region_phase_times) against tests/region_ref.py.

CPU tests pin the restatement on hand-built graphs, one per rule of the definition, and on the corner scene, and the argument checks answered on
the host.  GPU tests compare the HIP path with the restatement: labels, smooth mask, sizes and the three counts with np.array_equal, no
tolerance anywhere -- the result is a function of three predicates (curvature <= threshold, |ni . nj| >= min_abs_cos, d <= max_distance), which
numpy evaluates with the same roundings."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import features_ref as F
import region_ref as R
import test_outliers as TO
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T
from test_outliers import _code, _empty_buffer

NONE = 0xFFFFFFFF
N_ = NONE
PAD = -1
INF = float("inf")
BIG = 2 ** 64 - 1
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
THREADS = 256                                   # asserted against pst_region_kernel_shape below: the parametrisations need them at collection time
POINTS_PER_BLOCK = {1: 256, 3: 256, 16: 128, 64: 32}
COS10 = math.cos(math.radians(10.0))


def lists(rows, k):
    """(n, k) int64 from per-point lists, padded with -1"""
    out = np.full((len(rows), k), PAD, dtype=np.int64)
    for i, row in enumerate(rows):
        out[i, :len(row)] = row
    return out


def ref(knn, normals, curvature=None, positions=None, **kw):
    labels, sizes, smooth = R.region_growing(knn, np.asarray(normals, dtype=np.float64), curvature, positions, **kw)
    return labels.tolist(), sizes.tolist(), smooth.astype(int).tolist()


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_an_asymmetric_list_still_unites():
    """0 names 1 and 2 names 1; 1 names nobody.  4 names 5.  3 is named by nobody and names nobody."""
    knn = lists([[1], [], [1], [], [5], []], 1)
    assert ref(knn, [Z] * 6) == ([0, 0, 0, 2, 1, 1], [3, 2, 1], [1] * 6)


def test_a_rim_point_joins_its_first_agreeing_slot_not_the_nearest():
    """A = {0, 1} with normal Z, B = {2, 3} with normal X.  Point 4 (rim, normal (0.6, 0, 0.8): |dot| 0.8 with Z, 0.6 with X, both >= 0.5)
    lists 5 (a rim point: passed over), then 2 (B, two units away), then 0 (A, one unit away): it joins B.  Point 5 (rim, normal Z) lists 4
    twice (rim) and then 1: it joins A.  Both regions have three members; A holds the smaller index."""
    knn = lists([[1], [], [3], [], [5, 2, 0], [4, 4, 1]], 3)
    normals = [Z, Z, X, X, (0.6, 0.0, 0.8), Z]
    curvature = np.array([0, 0, 0, 0, 1, 1], dtype=np.float64)
    pos = np.array([[0, 0, 0], [0, 1, 0], [3, 0, 0], [3, 1, 0], [1, 0, 0], [1, 1, 0]], dtype=np.float64)
    for limit in (INF, 10.0):
        assert ref(knn, normals, curvature, pos, min_abs_cos=0.5, curvature_threshold=0.5, max_distance=limit) == ([0, 0, 1, 1, 1, 0], [3, 3], [1, 1, 1, 1, 0, 0])
    # within 1.5 point 4 no longer reaches 2 and falls to A
    assert ref(knn, normals, curvature, pos, min_abs_cos=0.5, curvature_threshold=0.5, max_distance=1.5) == ([0, 0, 1, 1, 0, 0], [4, 2], [1, 1, 1, 1, 0, 0])


def test_a_rim_point_does_not_bridge():
    """{0, 1} and {3, 4} both reach the rim point 2, and 2 lists both: it joins 1's region (its first slot) and the two stay apart.  Were 2
    smooth they would be one region.  Point 5 has a NaN normal: unlabelled whatever it lists."""
    knn = lists([[1], [2], [1, 3], [4, 2], [], [0, 1]], 2)
    normals = [Z, Z, Z, Z, Z, (np.nan, 0.0, 1.0)]
    curvature = np.array([0, 0, 1, 0, 0, 0], dtype=np.float64)
    assert ref(knn, normals, curvature, curvature_threshold=0.5) == ([0, 0, 0, 1, 1, N_], [3, 2], [1, 1, 0, 1, 1, 0])
    assert ref(knn, normals, None) == ([0, 0, 0, 0, 0, N_], [5], [1, 1, 1, 1, 1, 0])


def test_a_rim_point_without_an_agreeing_slot_is_unlabelled():
    """2: its smooth neighbours disagree.  3: lists only a rim point.  4: lists itself and an index out of range.  5: second slot agrees."""
    knn = lists([[1], [], [0, 1], [2], [4, 7], [2, 0]], 2)
    normals = [Z, Z, X, Z, Z, Z]
    curvature = np.array([0, 0, 1, 1, 1, 1], dtype=np.float64)
    assert ref(knn, normals, curvature, min_abs_cos=0.9, curvature_threshold=0.5) == ([0, 0, N_, N_, N_, 0], [3], [1, 1, 0, 0, 0, 0])


def test_a_point_with_a_normal_that_is_not_finite_is_unlabelled_and_nobodys_neighbour():
    knn = lists([[1], [2], [], [0], [3], [4]], 1)
    normals = [Z, (np.nan, 0.0, 1.0), Z, (0.0, np.inf, 0.0), Z, Z]
    assert ref(knn, normals) == ([1, N_, 2, N_, 0, 0], [2, 1, 1], [1, 0, 1, 0, 1, 1])


def test_a_nan_curvature_is_not_smooth():
    """1 (NaN) and 4 (just above the threshold) are rim points: 0 lists only 1 and stays alone; 1 and 4 join {2, 3}."""
    knn = lists([[1], [2], [], [2], [3], []], 1)
    curvature = np.array([0.0, np.nan, 0.0, 0.5, np.nextafter(0.5, 1.0), -np.inf])
    assert ref(knn, [Z] * 6, curvature, curvature_threshold=0.5) == ([1, 0, 0, 0, 0, 2], [4, 1, 1], [1, 0, 1, 1, 0, 1])


def test_self_and_out_of_range_slots_are_skipped():
    knn = lists([[0, 6, 0xFFFFFFFF, 2 ** 31 + 1], [1, 1, 1, 1], [2, 100, 3, 3], [], [], []], 4)
    assert ref(knn, [Z] * 6) == ([1, 2, 0, 0, 3, 4], [2, 1, 1, 1, 1], [1] * 6)


def test_the_size_filter():
    knn = lists([[1], [2], [3], [], [5], [], [], []], 1)
    assert ref(knn, [Z] * 8, min_size=2, max_size=3) == ([N_, N_, N_, N_, 0, 0, N_, N_], [2], [1] * 8)
    assert ref(knn, [Z] * 8, min_size=2) == ([0, 0, 0, 0, 1, 1, N_, N_], [4, 2], [1] * 8)
    assert ref(knn, [Z] * 8, max_size=1) == ([N_, N_, N_, N_, N_, N_, 0, 1], [1, 1], [1] * 8)
    assert ref(knn, [Z] * 8, min_size=5) == ([N_] * 8, [], [1] * 8)


def test_numbering_ties_go_to_the_smallest_member():
    knn = lists([[7], [], [3], [], [5], [6], [], [], [1]], 1)
    assert ref(knn, [Z] * 9) == ([1, 2, 3, 3, 0, 0, 0, 1, 2], [3, 2, 2, 2], [1] * 9)
    # the smallest member may be a rim point: {3, 4} with the rim point 0 comes before {1, 2, 5}
    knn = lists([[3], [2], [5], [4], [], []], 1)
    curvature = np.array([1, 0, 0, 0, 0, 0], dtype=np.float64)
    assert ref(knn, [Z] * 6, curvature, curvature_threshold=0.5) == ([0, 1, 1, 0, 0, 1], [3, 3], [0, 1, 1, 1, 1, 1])


def test_the_restatement_on_degenerate_input():
    labels, sizes, smooth = R.region_growing(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 3)))
    assert labels.shape == sizes.shape == smooth.shape == (0,)
    assert ref(lists([[1], [0]], 1), [(np.nan,) * 3] * 2) == ([N_, N_], [], [0, 0])


@functools.lru_cache(maxsize=None)
def corner():
    """(points, brute-force lists k = 16, normals, curvature of the restated features): computed once, read-only"""
    pts = R.corner_scene()
    knn = R.brute_knn(pts, 16)
    f = F.features(pts, knn)
    out = pts, knn, f["normals"], f["surface_variation"]
    for a in out:
        a.setflags(write=False)
    return out


def test_the_corner_scene_has_three_faces():
    """Three unit faces of 40 x 40 points, noise 0.002, k = 16, 10 degrees, curvature 0.02, min_size 100: the three faces and nothing else.
    The points along the edges have bent normals and a high curvature: they are rim points or fall into slivers below min_size."""
    pts, knn, normals, curvature = corner()
    labels, sizes, smooth = R.region_growing(knn, normals, curvature, min_abs_cos=COS10, curvature_threshold=0.02, min_size=100)
    print("corner scene: sizes", sizes.tolist(), "smooth", int(smooth.sum()))
    assert len(sizes) == 3 and (sizes >= 1400).all(), sizes
    for c in range(3):  # every region lies in one face
        assert len(np.unique(np.flatnonzero(labels == c) // 1600)) == 1
    slivers = R.region_growing(knn, normals, curvature, min_abs_cos=COS10, curvature_threshold=0.02)[1]
    print("corner scene at min_size 1: sizes", slivers.tolist())
    assert (slivers[:3] == sizes).all()


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def test_kernel_shape(hip):
    for k, p in POINTS_PER_BLOCK.items():
        assert alg.region_kernel_shape(k, hip) == {"points_per_block": p, "threads": THREADS}
        assert p * k % THREADS == 0
    one = C.c_uint32(7)
    hip.region_kernel_shape(8, None, C.byref(one))  # each pointer is optional
    assert one.value == THREADS
    hip.region_kernel_shape(64, None, None)
    for k in (0, 65):
        assert _code(lambda: hip.region_kernel_shape(k, None, None)) == 1
    assert alg.region_phase_times(hip) == (0.0, 0.0, 0.0)
    assert _code(lambda: hip.region_phase_times(None)) == 1


FAKE = C.c_void_p(8)  # never dereferenced: every call that takes it fails before that


def _from_knn(hip, counts, b, k=4, knn=FAKE, normals=FAKE, curvature=FAKE, cos=0.9, thr=0.1, limit=INF, lo=1, hi=BIG, labels=FAKE, smooth=FAKE, kind=1, sizes=None, cap=0):
    return hip.region_growing_from_knn(b, k, knn, normals, curvature, cos, thr, limit, lo, hi, labels, smooth, kind, sizes, cap, counts)


def _full(hip, counts, b, k=8, cos=0.9, thr=0.1, limit=INF, lo=1, hi=BIG, labels=FAKE, smooth=FAKE, kind=1, sizes=None, cap=0, normals=None, curvature=None, knn=None):
    return hip.region_growing(b, k, cos, thr, limit, lo, hi, labels, smooth, kind, sizes, cap, counts, normals, curvature, knn)


@pytest.mark.parametrize("entry", [_from_knn, _full])
def test_argument_errors_answered_on_the_host(hip, entry):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    counts = (C.c_uint64 * 3)()
    h = buf._h
    assert _code(lambda: entry(hip, counts, None)) == 1
    assert _code(lambda: entry(hip, counts, h, labels=None)) == 1
    assert _code(lambda: entry(hip, None, h)) == 1
    assert _code(lambda: entry(hip, counts, h, kind=7)) == 1  # no such memory kind
    for cos in (-0.5, float(np.nextafter(1.0, 2.0)), float("nan"), INF, -5e-324):
        assert _code(lambda: entry(hip, counts, h, cos=cos)) == 1, cos
    assert _code(lambda: entry(hip, counts, h, thr=float("nan"))) == 1
    for limit in (-1.0, float("nan"), -INF, -5e-324):
        assert _code(lambda: entry(hip, counts, h, limit=limit)) == 1, limit
    assert _code(lambda: entry(hip, counts, h, lo=0)) == 1
    assert _code(lambda: entry(hip, counts, h, lo=3, hi=2)) == 1
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: entry(hip, counts, f32._h)) == 4
    with pytest.raises(PasturePanic):
        entry(hip, counts, f32._h)
    if entry is _from_knn:
        assert _code(lambda: entry(hip, counts, h, knn=None)) == 1
        assert _code(lambda: entry(hip, counts, h, normals=None)) == 1
        for k in (0, 65, 2 ** 40):
            assert _code(lambda: entry(hip, counts, h, k=k)) == 1, k
    else:
        for k in (0, 1, 2):
            assert _code(lambda: entry(hip, counts, h, k=k)) == 12, k  # the search's own answer: k too small
        assert _code(lambda: entry(hip, counts, h, k=65)) == 23
    with pytest.raises(ValueError):
        alg.region_growing(buf, 8, device_smooth_ptr=8)  # a smooth mask in device memory needs the labels there too


def test_legal_parameters_and_an_empty_buffer_from_lists(hip):
    """The limits of every range are legal, a null curvature, smooth mask and sizes array too; an empty buffer is answered on the host, with
    or without a device: zero counts, nothing dereferenced."""
    for buf in (_empty_buffer(hip), _empty_buffer(hip, kind=VectorBuffer)):
        for kw in ({}, {"cos": 0.0, "thr": -INF, "limit": 0.0}, {"cos": 1.0, "thr": INF, "hi": 1}, {"k": 1, "curvature": None, "smooth": None}, {"k": 64, "kind": 0},
                   {"sizes": (C.c_uint64 * 2)(), "cap": 2}):
            counts = (C.c_uint64 * 3)(5, 5, 5)
            _from_knn(hip, counts, buf._h, **kw)
            assert list(counts) == [0, 0, 0]
    r = alg.region_growing_from_knn(_empty_buffer(hip), 4, np.zeros((0, 4), dtype=np.int64), np.zeros((0, 3)), np.zeros(0))
    assert r.labels.shape == r.smooth.shape == r.sizes.shape == (0,) and (r.n_smooth, r.n_labelled) == (0, 0)


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    labels, smooth = (C.c_uint32 * 8)(), (C.c_uint8 * 8)()
    for buf in (_empty_buffer(hip), _empty_buffer(hip, kind=VectorBuffer)):
        for kw in ({}, {"k": 3, "smooth": None}, {"k": 64, "limit": 2.5, "kind": 0}):
            with pytest.raises(PastureError) as e:
                _full(hip, (C.c_uint64 * 3)(), buf._h, **{"labels": labels, "smooth": smooth, **kw})
            assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------ GPU helpers

DIRECTIONS = np.array([X, Y, Z, (-1.0, 0.0, 0.0), (0.6, 0.8, 0.0), (0.8, 0.6, 0.0), (0.0, -0.6, 0.8)])


def synthetic(n, k, seed):
    """Random lists with padding, out-of-range, self and repeated entries; unit normals from a few directions (so agreement is frequent) with a
    few that are not finite; curvature in [0, 1) with a few NaNs; positions on a dyadic lattice"""
    rng = np.random.default_rng(seed)
    knn = rng.integers(0, n, (n, k), dtype=np.int64)
    kind = rng.random((n, k))
    knn[kind < 0.10] = PAD
    knn[(kind >= 0.10) & (kind < 0.15)] = n + rng.integers(0, 9)
    knn[(kind >= 0.15) & (kind < 0.18)] = 2 ** 31 + 3
    own = (kind >= 0.18) & (kind < 0.24)
    knn[own] = np.broadcast_to(np.arange(n)[:, None], (n, k))[own]
    if k > 1:
        again = kind[:, 1] > 0.8
        knn[again, 1] = knn[again, 0]
    normals = DIRECTIONS[rng.integers(0, len(DIRECTIONS), n)].copy()
    bad = rng.random(n)
    normals[bad < 0.04, rng.integers(0, 3)] = np.nan
    normals[(bad >= 0.04) & (bad < 0.06), rng.integers(0, 3)] = -np.inf
    curvature = rng.random(n)
    curvature[rng.random(n) < 0.05] = np.nan
    positions = rng.integers(0, 16, (n, 3)).astype(np.float64) * 0.25
    return knn, normals, curvature, positions


def gpu_from_knn(hip, knn, normals, curvature=None, positions=None, storage="H", device=False, want_smooth=True, **kw):
    """(labels, sizes, smooth, (regions, n_smooth, n_labelled)) of the from-lists entry through host or device memory"""
    n, k = knn.shape
    buf = TO.make_buffer(hip, positions if positions is not None else np.zeros((n, 3)), storage)
    if not device:
        r = alg.region_growing_from_knn(buf, k, knn, normals, curvature, return_smooth=want_smooth, **kw)
        assert r.labels.dtype == np.uint32 and r.sizes.dtype == np.uint64 and r.labels.shape == (n,)
        assert (r.smooth is None) if not want_smooth else (r.smooth.dtype == bool and r.smooth.shape == (n,))
        return r.labels, r.sizes, r.smooth, (len(r.sizes), r.n_smooth, r.n_labelled)
    import torch
    dl = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ds = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    r = alg.region_growing_from_knn(buf, k, knn, normals, curvature, device_labels_ptr=dl.data_ptr(), device_smooth_ptr=ds.data_ptr() if want_smooth else None, **kw)
    assert r.labels is None and r.smooth is None
    smooth = ds.cpu().numpy()
    assert want_smooth or (smooth == 7).all(), "a null smooth pointer: nothing is written"
    return dl.cpu().numpy().view(np.uint32), r.sizes, smooth.astype(bool) if want_smooth else None, (len(r.sizes), r.n_smooth, r.n_labelled)


def assert_same(got, want, what=""):
    gl, gs, gm, counts = got
    wl, ws, wm = want
    assert np.array_equal(gs, ws), f"{what}: sizes {gs[:8]} ({len(gs)}) vs {ws[:8]} ({len(ws)})"
    bad = np.flatnonzero(gl != wl)
    assert bad.size == 0, f"{what}: {bad.size} of {len(wl)} labels differ, first at {bad[:4]}: {gl[bad[:4]]} vs {wl[bad[:4]]}"
    if gm is not None:
        bad = np.flatnonzero(gm != wm)
        assert bad.size == 0, f"{what}: {bad.size} of {len(wm)} smooth flags differ, first at {bad[:4]}"
    assert counts == (len(ws), int(wm.sum()), int((wl != NONE).sum())), f"{what}: counts {counts}"


def seam_lengths(k):
    """1, 2, the wave, the workgroup's points and the lengths whose LAST workgroup owns a whole number of 256-element passes, one less and one more"""
    p = POINTS_PER_BLOCK[k]
    ns = {1, 2, 63, 64, 65, p - 1, p, p + 1, 2 * p + 1}
    for passes in (1, 2):
        r = -(-passes * THREADS // k)  # the fewest points whose elements fill the passes
        ns |= {p + r + d for d in (-1, 0, 1) if 0 < r + d < p}
    return sorted(ns)


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 16, 64])
def test_lengths_around_the_seams(hip, k):
    assert alg.region_kernel_shape(k, hip) == {"points_per_block": POINTS_PER_BLOCK[k], "threads": THREADS}
    for t, n in enumerate(seam_lengths(k)):
        knn, normals, curvature, positions = synthetic(n, k, 100 * k + t)
        # in turn: no curvature and no limit; curvature; curvature, a limit and a size filter
        kw = [dict(min_abs_cos=0.9), dict(min_abs_cos=0.75, curvature_threshold=0.7), dict(min_abs_cos=0.9, curvature_threshold=0.6, max_distance=2.5, min_size=2, max_size=n // 2 + 2)][t % 3]
        curv = None if t % 3 == 0 else curvature
        want = R.region_growing(knn, normals, curv, positions, **kw)
        got = gpu_from_knn(hip, knn, normals, curv, positions, storage="H" if t % 2 else "V", device=t % 4 == 1, **kw)
        assert_same(got, want, f"k {k} n {n} {kw}")


def _knife_cos():
    """dot = (1 * 0.5 + 0 * 0.5) + 0 * 0 = 0.5 exactly, once with either sign: 0 and 1 join iff min_abs_cos <= 0.5"""
    for sign in (1.0, -1.0):
        for cos in (0.5, float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))):
            yield dict(normals=[X, (0.5 * sign, 0.5, 0.0)], kw=dict(min_abs_cos=cos), joined=cos <= 0.5)


def _knife_curvature():
    """point 1 is smooth iff 0.25 <= threshold: then 0 - 1 - 2 is one region; as a rim point it joins 2, the only point it lists, and 0 stays alone"""
    for thr in (0.25, float(np.nextafter(0.25, 0.0)), float(np.nextafter(0.25, 1.0))):
        yield dict(normals=[Z, Z, Z], curvature=[0.0, 0.25, 0.0], knn=[[1], [2], []], kw=dict(curvature_threshold=thr), regions=1 if thr >= 0.25 else 2)


def _knife_distance():
    """the slot's own distance and one ulp either side: 1.25 = sqrt((0.75^2 + 1^2) + 0) exactly, sqrt(0.75) rounded"""
    for p1 in ((0.75, 1.0, 0.0), (0.5, 0.5, 0.5)):
        pos = np.array([(0.0, 0.0, 0.0), p1])
        d = float(np.sqrt((pos[1, 0] * pos[1, 0] + pos[1, 1] * pos[1, 1]) + pos[1, 2] * pos[1, 2]))
        for limit in (d, float(np.nextafter(d, 0.0)), float(np.nextafter(d, INF))):
            yield dict(normals=[Z, Z], positions=pos + 8.0 if p1[2] == 0.0 else pos, kw=dict(max_distance=limit), joined=limit >= d)


@pytest.mark.gpu
@pytest.mark.parametrize("family", [_knife_cos, _knife_curvature, _knife_distance])
def test_knife_edges(hip, family):
    for case in family():
        normals = np.array(case["normals"], dtype=np.float64)
        n = len(normals)
        knn = lists(case.get("knn", [[1], []]), 1)
        curvature = np.array(case["curvature"]) if "curvature" in case else None
        positions = case.get("positions")
        want = R.region_growing(knn, normals, curvature, positions, **case["kw"])
        regions = case["regions"] if "regions" in case else 1 if case["joined"] else 2
        assert len(want[1]) == regions, (case, want)
        for device in (False, True):
            assert_same(gpu_from_knn(hip, knn, normals, curvature, positions, device=device, **case["kw"]), want, f"{case}")
        # the same edge found by the attach kernel: point 0 as a rim point that names 1
        if family is not _knife_curvature:
            rim = np.array([1.0] + [0.0] * (n - 1))
            want = R.region_growing(knn, normals, rim, positions, curvature_threshold=0.5, **case["kw"])
            assert int((want[0] != NONE).sum()) == (2 if case["joined"] else 1), (case, want)
            assert_same(gpu_from_knn(hip, knn, normals, rim, positions, curvature_threshold=0.5, **case["kw"]), want, f"rim {case}")


N_STRUCTURE = 200_003


def _structure(name):
    n = N_STRUCTURE
    rng = np.random.default_rng(11)
    normals = np.broadcast_to(np.array(Z), (n, 3))
    curvature = None
    if name == "one_region_shuffled":   # a ring through a random permutation, every point names its successor and its predecessor
        perm = rng.permutation(n)
        knn = np.empty((n, 2), dtype=np.int64)
        knn[perm, 0] = np.roll(perm, -1)
        knn[perm, 1] = np.roll(perm, 1)
        expect = 1
    elif name == "every_point_alone":   # lists that name nothing but the point itself or nobody: more than kFoldRounds roots in every wave
        knn = np.where(rng.random((n, 2)) < 0.5, np.arange(n)[:, None], PAD)
        expect = n
    elif name == "path":                # lists that name only i + 1
        knn = (np.arange(n, dtype=np.int64) + 1)[:, None].copy()
        knn[-1, 0] = PAD
        expect = 1
    else:                               # 1 000 regions of 200 points, i in region i % 1000, and three left over
        knn = (np.arange(n, dtype=np.int64) + 1000)[:, None].copy()
        knn[knn >= 200_000] = PAD
        knn[200_000:] = PAD
        expect = 1003
    return knn, normals, curvature, expect


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_region_shuffled", "every_point_alone", "path", "equal_regions"])
def test_structure_at_200003_points(hip, name):
    knn, normals, curvature, expect = _structure(name)
    want = R.region_growing(knn, normals, curvature, curvature_threshold=0.5)
    assert len(want[1]) == expect
    got = gpu_from_knn(hip, knn, normals, curvature, curvature_threshold=0.5, device=name == "path")
    assert_same(got, want, name)
    if name == "equal_regions":
        assert np.array_equal(want[0][:200_000], np.arange(200_000) % 1000) and want[1][:1000].tolist() == [200] * 1000
        want = R.region_growing(knn, normals, None, min_size=2, max_size=200)
        assert len(want[1]) == 1000 and (want[0][200_000:] == NONE).all()
        assert_same(gpu_from_knn(hip, knn, normals, None, min_size=2, max_size=200), want, name + " filtered")


@pytest.mark.gpu
def test_determinism_and_outputs(hip):
    import torch
    n, k = 5000, 8
    knn, normals, curvature, positions = synthetic(n, k, 77)
    kw = dict(min_abs_cos=0.75, curvature_threshold=0.7, max_distance=3.0)
    want = R.region_growing(knn, normals, curvature, positions, **kw)
    assert len(want[1]) > 10
    runs = [gpu_from_knn(hip, knn, normals, curvature, positions, storage=s, device=d, want_smooth=m, **kw)
            for s, d, m in (("H", False, True), ("H", False, True), ("V", True, True), ("packedV", False, False), ("H", True, False))]
    for got in runs:
        assert_same(got, want)
        assert got[0].tobytes() == runs[0][0].tobytes() and got[1].tobytes() == runs[0][1].tobytes()
    # a size array that is too small: PST_ERR_RANGE with the counts set and the labels written
    buf = TO.make_buffer(hip, positions, "H")
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(t).cuda()  # noqa: E731
    dk = torch.from_numpy((knn & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
    dn, dc = dev(normals, torch.float64), dev(curvature, torch.float64)
    labels, smooth, sizes, counts = np.full(n, 7, dtype=np.uint32), np.full(n, 7, dtype=np.uint8), np.zeros(3, dtype=np.uint64), (C.c_uint64 * 3)()
    args = (buf._h, k, C.c_void_p(dk.data_ptr()), C.c_void_p(dn.data_ptr()), C.c_void_p(dc.data_ptr()), 0.75, 0.7, 3.0, 1, BIG, C.c_void_p(labels.ctypes.data),
            C.c_void_p(smooth.ctypes.data), 1, sizes.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert _code(lambda: hip.region_growing_from_knn(*args, 3, counts)) == 3
    assert list(counts) == [len(want[1]), int(want[2].sum()), int((want[0] != NONE).sum())]
    assert np.array_equal(labels, want[0]) and np.array_equal(smooth.astype(bool), want[2]) and not sizes.any()
    # a cloud without a valid normal
    nothing = np.full((n, 3), np.nan)
    got = gpu_from_knn(hip, knn, nothing, curvature, positions, **kw)
    assert_same(got, R.region_growing(knn, nothing, curvature, positions, **kw))
    assert got[3] == (0, 0, 0) and (got[0] == NONE).all() and not got[2].any()


@functools.lru_cache(maxsize=None)
def sphere():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(3000, 3))
    pts = v / np.linalg.norm(v, axis=1)[:, None] * (1.0 + rng.normal(0.0, 0.01, 3000))[:, None] + 100.0
    pts.setflags(write=False)
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "V"])
@pytest.mark.parametrize("scene", ["corner", "sphere"])
def test_the_full_call(hip, scene, storage):
    """Search, features and regions in one call: equal to the restatement applied to the lists, normals and curvature the call itself returned,
    and byte for byte what the from-lists entry makes of them."""
    pts = corner()[0] if scene == "corner" else sphere()
    k = 16 if scene == "corner" else 10
    kw = dict(min_abs_cos=COS10, curvature_threshold=0.02, min_size=100) if scene == "corner" else dict(min_abs_cos=math.cos(math.radians(15.0)), curvature_threshold=0.05, max_distance=0.12)
    buf = TO.make_buffer(hip, pts, storage)
    r = alg.region_growing(buf, k, return_inputs=True, **kw)
    n = len(pts)
    assert r.knn.shape == (n, k) and r.normals.shape == (n, 3) and r.curvature.shape == (n,)
    want = R.region_growing(r.knn, r.normals, r.curvature, pts, **kw)
    print(scene, "sizes", r.sizes[:8].tolist(), "regions", len(r.sizes), "smooth", r.n_smooth, "labelled", r.n_labelled)
    assert_same((r.labels, r.sizes, r.smooth, (len(r.sizes), r.n_smooth, r.n_labelled)), want, scene)
    again = alg.region_growing_from_knn(buf, k, r.knn, r.normals, r.curvature, **kw)
    assert again.labels.tobytes() == r.labels.tobytes() and again.sizes.tobytes() == r.sizes.tobytes() and again.smooth.tobytes() == r.smooth.tobytes()
    assert (again.n_smooth, again.n_labelled) == (r.n_smooth, r.n_labelled)
    plain = alg.region_growing(buf, k, **kw)  # nothing handed back: the same regions from scratch memory
    assert plain.labels.tobytes() == r.labels.tobytes() and plain.sizes.tobytes() == r.sizes.tobytes() and plain.normals is None
    if scene == "corner":
        assert len(r.sizes) == 3 and (r.sizes >= 1300).all(), r.sizes
        by_degrees = alg.region_growing(buf, k, smoothness_deg=10.0, curvature_threshold=0.02, min_size=100)
        assert by_degrees.labels.tobytes() == r.labels.tobytes()
    else:
        assert r.n_smooth > 0 and len(r.sizes) > 0


@pytest.mark.gpu
def test_too_few_points_and_an_empty_buffer_in_the_full_call(hip):
    r = alg.region_growing(_empty_buffer(hip), 8)
    assert r.labels.shape == r.sizes.shape == (0,) and (r.n_smooth, r.n_labelled) == (0, 0)
    for n in (1, 2):
        buf = TO.make_buffer(hip, np.arange(3.0 * n).reshape(n, 3), "H")
        assert _code(lambda: alg.region_growing(buf, 3)) == 11


@pytest.mark.gpu
def test_extract_regions(hip):
    pts = corner()[0]
    kw = dict(min_abs_cos=COS10, curvature_threshold=0.02, min_size=100)
    buf = TO.make_buffer(hip, pts, "H")
    r = alg.region_growing(buf, 16, **kw)
    from pasture_amd.layout import attributes as A
    for first, count in ((0, 1), (1, 2), (0, 0xFFFFFFFF), (2, 5), (3, 1)):
        out, sizes = alg.extract_regions(buf, 16, first_region=first, region_count=count, **kw)
        assert np.array_equal(sizes, r.sizes)
        keep = (r.labels != NONE) & (r.labels >= first) & (r.labels.astype(np.int64) - first < count)
        assert out.len() == int(keep.sum())
        got = out.view_attribute(A.POSITION_3D) if out.len() else np.zeros((0, 3))
        assert np.asarray(got).reshape(-1, 3).tobytes() == pts[keep].tobytes(), (first, count)


@pytest.mark.gpu
def test_the_example_finds_the_four_roof_faces():
    """examples/roof_planes.py: the four largest regions are the four roof faces, one each; DBSCAN makes one blob of a house, both faces in it."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("roof_planes", os.path.join(root, "examples", "roof_planes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.main(40000)
    assert sorted(r["region_faces"]) == [[0], [1], [2], [3]], r
    # A neighbourhood of k = 16 points at SPACING 0.25 has a radius of about sqrt(16 / pi) * 0.25 = 0.56: a point closer than that to the ridge,
    # the eaves or a gable end may see the other face or a wall, bend its normal and raise its curvature.  The points farther in cannot, and they
    # are (14 - 1.13) * (4.72 - 1.13) / (14 * 4.72) = 0.70 of the first house's faces and (10 - 1.13) * (5.83 - 1.13) / (10 * 5.83) = 0.71 of the second's.
    assert all(size >= 0.70 * planted for size, planted in zip(sorted(r["region_sizes"][:4]), sorted(r["planted"]))), r
    assert sorted(sorted(f) for f in r["dbscan_faces"][:2]) == [[0, 1], [2, 3]], r
    assert r["roof_points"] == sum(r["region_sizes"][:4])
