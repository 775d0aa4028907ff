"""Geometric features from the kNN covariance eigenvalues (pst_geometric_features_from_knn_device, pst_geometric_features) against
tests/features_ref.py.

CPU tests pin the restatement against np.linalg.eigh on the eleven cloud families, on hand-computed clouds, and the argument checks answered on
the host.  GPU tests compare the HIP kernel with the restatement as u64 views, without a tolerance; OMNIVARIANCE and EIGENENTROPY alone carry
a bound in ulp (derived in compare()).  The kernel is driven through the from-lists entry with lists from tests/outlier_ref.py, so that no
tie-break of the search is involved; the full call is then compared with the from-lists entry fed with the lists it returned."""
import ctypes as C
import math

import numpy as np
import pytest

import features_ref as F
import outlier_ref as R
import test_outliers as TO
from pasture_amd import PastureError
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

INF = float("inf")
EIGH_BOUND = 32 * 2.0 ** -52
SEAM_KS = [3, 4, 8, 9, 10, 16, 17, 32, 33, 63, 64]   # the issue's k, and both sides of every k at which points_per_block changes (asserted below)


def P(k):
    """points per workgroup at this k, from the library (host only: no device is needed)"""
    return alg.features_kernel_shape(k)["points_per_block"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


_CLOUDS = {}


def family_cloud(name, n, k):
    """(points, lists (n, k) int64 with -1 padding) of one family: the lists are searched before the family's scale factor is applied.
    Computed once and left unchanged."""
    key = (name, n, k)
    if key not in _CLOUDS:
        base, factor = F.family(name, n)
        idx, _ = R.knn(base, k)
        pts = base * factor
        for a in (pts, idx):
            a.setflags(write=False)
        _CLOUDS[key] = (pts, idx)
    return _CLOUDS[key]


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

@pytest.mark.parametrize("name", F.FAMILIES)
def test_restatement_against_eigh(name):
    """The Jacobi recipe against LAPACK on 2 * 10^3 neighbourhoods per family: sorted eigenvalues within 32 * 2^-52 * l1, |Cv - lambda v| within
    the same per component, and no family needs more than 6 sweeps."""
    k = 3 if name == "k3" else 10
    pts, idx = family_cloud(name, 2000, k)
    r = F.features(pts, idx)
    ok = (r["count"] >= 3) & (r["eigenvalue_1"] > 0.0)
    assert ok.sum() >= 1900, "the family is meant to give proper neighbourhoods"
    c = r["cov"][ok]
    # (LAPACK is given the matrix scaled by a power of two, which is exact and keeps its own arithmetic in range at 10^-300 and 10^300)
    scale = 2.0 ** np.floor(np.log2(np.abs(c).max(axis=1)))
    cs = c / scale[:, None]
    M = np.stack([cs[:, [0, 1, 2]], cs[:, [1, 3, 4]], cs[:, [2, 4, 5]]], axis=1)
    want = np.linalg.eigvalsh(M)[:, ::-1]
    lam = np.stack([r["eigenvalue_1"], r["eigenvalue_2"], r["eigenvalue_3"]], axis=1)[ok] / scale[:, None]
    l1 = lam[:, 0]
    assert np.all(lam[:, 0] >= lam[:, 1]) and np.all(lam[:, 1] >= lam[:, 2]) and np.all(lam[:, 2] >= 0.0)
    dev = np.abs(lam - want).max(axis=1) / l1
    vecs = [r["directions"][ok], r["e2"][ok], r["normals"][ok]]
    res = max(float((np.abs(np.einsum("nij,nj->ni", M, v) - lam[:, i:i + 1] * v).max(axis=1) / l1).max()) for i, v in enumerate(vecs))
    print(f"{name}: eigenvalue deviation {dev.max():.3g}, residual {res:.3g} of l1 (bound {EIGH_BOUND:.3g}), sweeps <= {r['sweeps'].max()}")
    assert dev.max() <= EIGH_BOUND
    assert res <= EIGH_BOUND
    assert r["sweeps"].max() <= 6
    for v in vecs:
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 4 * 2.0 ** -52


def test_restatement_on_hand_computed_clouds():
    nan_bits = bits(F.CANONICAL_NAN)
    # the 3 x 3 unit lattice in z = 0, every list naming all nine points: variance (1 + 0 + 1) * 3 / 9 = 2/3 in x and y, nothing else
    lattice = np.array([[x, y, 0.0] for x in range(3) for y in range(3)])
    r = F.features(lattice, np.tile(np.arange(9), (9, 1)))
    for name, want in (("eigenvalue_1", 2.0 / 3.0), ("eigenvalue_2", 2.0 / 3.0), ("eigenvalue_3", 0.0), ("linearity", 0.0), ("planarity", 1.0), ("scattering", 0.0),
                       ("anisotropy", 1.0), ("surface_variation", 0.0), ("eigenvalue_sum", 2.0 / 3.0 + 2.0 / 3.0), ("verticality", 0.0), ("omnivariance", 0.0),
                       ("eigenentropy", math.log(2.0)), ("count", 9.0)):
        assert np.array_equal(bits(r[name]), bits(np.full(9, want))), name
    assert np.array_equal(bits(r["normals"]), bits(np.tile([0.0, 0.0, 1.0], (9, 1)))) and not r["sweeps"].any()
    # three points on the x axis: variance (1 + 0 + 1) / 3
    line = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    r = F.features(line, np.tile(np.arange(3), (3, 1)))
    assert np.array_equal(r["eigenvalue_1"], [2.0 / 3.0] * 3) and not r["eigenvalue_2"].any() and not r["eigenvalue_3"].any()
    assert np.array_equal(r["linearity"], [1.0] * 3) and np.array_equal(bits(r["directions"]), bits(np.tile([1.0, 0.0, 0.0], (3, 1))))
    assert np.array_equal(r["planarity"], [0.0] * 3) and np.array_equal(r["count"], [3.0] * 3)
    # three coincident points: eigenvalues and their sum +0.0, every ratio and both vectors the canonical NaN
    r = F.features(np.full((3, 3), 4.5), np.tile(np.arange(3), (3, 1)))
    for name in F.NAMES:
        want = 0.0 if name.startswith("eigenvalue") else 3.0 if name == "count" else F.CANONICAL_NAN
        assert np.array_equal(bits(r[name]), bits(np.full(3, want))), name
    assert np.all(bits(r["normals"]) == nan_bits) and np.all(bits(r["directions"]) == nan_bits)
    # m = 2: everything but COUNT is the NaN -- by a short list, by padding, by an index out of range and by the distance limit
    for knn, limit in ((np.tile(np.arange(2), (3, 1)), INF), (np.array([[0, 1, -1], [1, 0, -1], [2, 0, -1]]), INF), (np.array([[0, 1, 3], [1, 0, 4], [2, 0, 3]]), INF),
                       (np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]]), 1.0)):
        r = F.features(line, knn, limit)
        assert np.array_equal(r["count"], [2.0, 2.0, 2.0] if limit == INF else [2.0, 3.0, 2.0])
        two = r["count"] == 2.0
        for name in F.NAMES[:-1]:
            assert np.all(bits(r[name])[two] == nan_bits), name
        assert np.all(bits(r["normals"])[two] == nan_bits)
    # orientation: unary minus of every component, so a zero becomes -0.0
    assert np.array_equal(bits(F._oriented(np.array([0.0, 0.0, 1.0, -1.0]), np.array([0.0, -1.0, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0, 0.0]))),
                          bits(np.array([[-0.0, -0.0, 1.0], [-0.0, 1.0, -0.0], [1.0, 0.0, 0.0], [1.0, -0.0, -0.0]])))


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64):
    return HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def test_kernel_shape(hip):
    """At least two workgroups' tiles (P * k * 24 bytes, rows padded to an odd number of doubles) fit the 160 KiB of LDS of a compute unit, and
    SEAM_KS holds both sides of every k at which P changes."""
    changes = set()
    for k in range(1, 65):
        shape = alg.features_kernel_shape(k, hip)
        assert shape["threads"] == 256 and 1 <= shape["points_per_block"] <= shape["threads"]
        assert 2 * shape["points_per_block"] * ((3 * k) | 1) * 8 <= 160 * 1024
        if k > 1 and P(k) != P(k - 1):
            changes |= {k - 1, k}
    assert changes <= set(SEAM_KS) and {3, 4, 10, 16, 17, 32, 33, 63, 64} <= set(SEAM_KS)
    one = C.c_uint32()
    hip.features_kernel_shape(10, None, C.byref(one))  # each pointer is optional
    assert one.value == 256
    hip.features_kernel_shape(10, None, None)
    for k in (0, 65):
        assert _code(lambda: hip.features_kernel_shape(k, None, None)) == 1


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that, or the buffer is empty
    full = hip.geometric_features
    lists = hip.geometric_features_from_knn_device
    assert _code(lambda: full(None, 10, INF, 8, fake, None, None, None)) == 1
    assert _code(lambda: lists(None, 10, fake, INF, 8, fake, None, None)) == 1
    assert _code(lambda: lists(buf._h, 10, None, INF, 8, fake, None, None)) == 1            # the lists are the input
    assert _code(lambda: full(buf._h, 2, INF, 8, fake, None, None, None)) == 12             # k < 3
    assert _code(lambda: full(buf._h, 65, INF, 8, fake, None, None, None)) == 23            # k > 64
    for k in (0, 65):
        assert _code(lambda: lists(buf._h, k, fake, INF, 8, fake, None, None)) == 1
    for features in (0, 8192):
        assert _code(lambda: full(buf._h, 10, INF, features, fake, None, None, None)) == 1
        assert _code(lambda: lists(buf._h, 10, fake, INF, features, fake, None, None)) == 1
    for limit in (float("nan"), -1.0):
        assert _code(lambda: full(buf._h, 10, limit, 8, fake, None, None, None)) == 1
        assert _code(lambda: lists(buf._h, 10, fake, limit, 8, fake, None, None)) == 1
    assert _code(lambda: full(buf._h, 10, INF, 8, None, None, None, None)) == 1              # none of the three outputs
    assert _code(lambda: lists(buf._h, 10, fake, INF, 8, None, None, None)) == 1
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: full(f32._h, 10, INF, 8, fake, None, None, None)) == 4
    assert _code(lambda: lists(f32._h, 10, fake, INF, 8, fake, None, None)) == 4
    # an empty buffer in the from-lists call is answered on the host, whichever outputs are asked for
    for k in (1, 64):
        assert lists(buf._h, k, fake, 0.0, F.ALL, fake, fake, fake) == 0
        assert lists(buf._h, k, fake, INF, 1, None, None, fake) == 0
    with pytest.raises(ValueError):
        alg.geometric_features(buf, 10, features=("roundness",))


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    buf = _empty_buffer(hip)
    fake = C.c_void_p(8)
    for k, limit, features, out in ((3, INF, 1, (fake, None, None, None)), (64, 0.0, F.ALL, (fake, fake, fake, fake)), (10, 2.5, 4096, (None, fake, None, None)),
                                    (10, INF, 512, (None, None, fake, None))):
        with pytest.raises(PastureError) as e:
            hip.geometric_features(buf._h, k, limit, features, *out)
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

SENTINEL = -7.0   # what the output arrays hold before the call


def gpu_features(hip, pts, knn, features=F.ALL, max_distance=INF, storage="H", out=True, normals=True, directions=True, buffer=None):
    """The from-lists entry: (planes (planes, n) or None, normals (n, 3) or None, directions (n, 3) or None)"""
    import torch
    buf = buffer if buffer is not None else TO.make_buffer(hip, pts, storage)
    n, k = knn.shape
    assert buf.len() == n
    lists = torch.from_numpy((np.asarray(knn).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy()).cuda()
    planes = bin(features).count("1")
    o = torch.full((planes, n), SENTINEL, dtype=torch.float64, device="cuda") if out else None
    nr = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda") if normals else None
    dr = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda") if directions else None
    ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
    alg.geometric_features_device(buf, k, features, ptr(o), max_distance, ptr(nr), ptr(dr), lists.data_ptr(), from_knn=True)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    return host(o), host(nr), host(dr)


def ulps(got, want):
    """the largest distance in units of the last place; NaNs must agree bit for bit"""
    g, w = bits(got).astype(np.int64), bits(want).astype(np.int64)
    nan = np.isnan(want)
    assert np.array_equal(g[nan], w[nan])
    return int(np.abs(g[~nan] - w[~nan]).max()) if (~nan).any() else 0


WORST = {"omnivariance": 0, "eigenentropy": 0}


def compare(got, ref, features=F.ALL, what=""):
    """`got` as gpu_features returns it against the restatement's dict: u64 views, no tolerance, with two exceptions.

    OMNIVARIANCE within 4 ulp: its argument (e_1 * e_2) * e_3 is made of separately rounded operations and is bit-identical on both sides; the
    device library and glibc each document cbrt within 1 ulp of the true value, so the two results are at most 2 ulp apart; twice that.
    EIGENENTROPY within 8 ulp: each e_i is bit-identical; the two logs are at most 2 ulp apart, and so are the products e_i * log(e_i) up to
    their own rounding (half an ulp on either side: 3 ulp of the term at most); the three terms -e_i * log(e_i) are all >= 0, so the sum has no
    cancellation and an error of 3 ulp in each term is at most 3 ulp of the sum, plus the half ulp of each of the two additions on either
    side where an operand differs: 4 ulp; twice that.
    Seen on an MI355X over this whole file: 3 ulp and 2 ulp.  Three is more than two results within 1 ulp of the true
    value can be apart, so one of the two cbrt does not keep its documented bound everywhere; the factor of two covers it."""
    planes, normals, directions = got
    if planes is not None:
        want = F.planes(ref, features)
        assert planes.shape == want.shape, what
        names = [name for name in F.NAMES if features & F.BITS[name]]
        for t, name in enumerate(names):
            if name in WORST:
                u = ulps(planes[t], want[t])
                WORST[name] = max(WORST[name], u)
                assert u <= (4 if name == "omnivariance" else 8), f"{what} {name}: {u} ulp"
            else:
                bad = np.flatnonzero(bits(planes[t]) != bits(want[t]))
                assert bad.size == 0, f"{what} {name}: {bad.size} of {want.shape[1]} differ, first {bad[:3]}: {planes[t][bad[:3]]!r} vs {want[t][bad[:3]]!r}"
    for name, v in (("normals", normals), ("directions", directions)):
        if v is not None:
            bad = np.flatnonzero((bits(v) != bits(ref[name])).any(axis=1))
            assert bad.size == 0, f"{what} {name}: {bad.size} rows differ, first {bad[:3]}: {v[bad[:3]]!r} vs {ref[name][bad[:3]]!r}"


def check(hip, pts, knn, max_distance=INF, what="", **kw):
    ref = F.features(pts, knn, max_distance)
    got = gpu_features(hip, pts, knn, max_distance=max_distance, **kw)
    compare(got, ref, what=what)
    return ref, got


def _seam_cases():
    return [(k, n) for k in SEAM_KS for n in sorted({3, P(k) - 1, P(k), P(k) + 1, 2 * P(k) + 1})]


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("k,n", _seam_cases())
def test_size_and_k_seams(hip, k, n):
    """Every family at the workgroup's seams; n < k pads the lists."""
    for name in F.FAMILIES:
        pts, idx = family_cloud(name, n, k)
        ref, _ = check(hip, pts, idx, what=f"{name} n={n} k={k}")
        assert ref["count"].max() == min(n, k)
    print("largest deviation so far, ulp:", WORST)


@pytest.mark.gpu
def test_overflowing_covariance(hip):
    """Coordinates at 10^155: the squared deviations overflow, the scale is not finite, everything but COUNT is the NaN."""
    base, _ = F.family("volume", 300)
    idx, _ = R.knn(base, 10)
    pts = base * 1e155
    ref, (planes, normals, directions) = check(hip, pts, idx)
    assert np.all(planes[12] == 10.0) and np.isnan(planes[:12]).all() and np.isnan(normals).all() and np.isnan(directions).all()
    assert np.all(bits(planes[:12]) == bits(F.CANONICAL_NAN))


@pytest.mark.gpu
def test_non_finite_points(hip):
    """NaN and +-inf points are skipped as neighbours and have m = 0 as queries."""
    base, _ = F.family("volume", 600)
    pts = base.copy()
    rng = np.random.default_rng(3)
    bad = rng.choice(600, 60, replace=False)
    pts[bad, rng.integers(0, 3, 60)] = rng.choice([np.nan, np.inf, -np.inf], 60)
    idx, _ = R.knn(base, 12)   # lists of the clean cloud: they name the spoilt points
    ref, (planes, _, _) = check(hip, pts, idx)
    good = np.isfinite(pts).all(axis=1)
    assert not planes[12][~good].any() and np.isnan(planes[:12][:, ~good]).all()
    assert planes[12][good].min() < 12 and planes[12][good].max() == 12 and np.isfinite(planes[0][good & (planes[12] >= 3)]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_padded_lists(hip, n):
    pts, idx = family_cloud("volume", n, 8)
    assert (idx[:, n:] == -1).all()
    ref, (planes, _, _) = check(hip, pts, idx)
    assert np.all(planes[12] == n)


@pytest.mark.gpu
def test_shuffled_lists_follow_slot_order(hip):
    pts, idx = family_cloud("utm", 500, 16)
    rng = np.random.default_rng(5)
    shuffled = np.stack([row[rng.permutation(16)] for row in idx])
    ref, _ = check(hip, pts, shuffled)
    # the order matters to the last bits (else this test would show nothing)
    assert (bits(ref["eigenvalue_3"]) != bits(F.features(pts, idx)["eigenvalue_3"])).any()


@pytest.mark.gpu
def test_repeated_and_out_of_range_indices(hip):
    """A repeated index counts every time; the indices n and n + 1 are skipped (only those two are used: a missing guard would show as wrong
    bytes from the neighbouring allocation at worst)."""
    n = 400
    pts, idx = family_cloud("volume", n, 10)
    rep = idx.copy()
    rep[:, 3] = rep[:, 1]
    rep[::3, 7] = rep[::3, 0]
    ref, (planes, _, _) = check(hip, pts, rep, what="repeated")
    assert np.all(planes[12] == 10)
    oor = idx.copy()
    oor[::2, 4] = n
    oor[1::3, 9] = n + 1
    oor[5::7, 0] = n
    ref, (planes, _, _) = check(hip, pts, oor, what="out of range")
    assert np.array_equal(planes[12], 10 - (oor >= n).sum(axis=1)) and planes[12].min() == 7  # (rows where the three patterns meet)
    # a list of nothing else: m = 0
    none = np.where(np.arange(n)[:, None] % 2 == 0, n, n + 1) + np.zeros((n, 10), dtype=np.int64)
    ref, (planes, normals, _) = check(hip, pts, none, what="all out of range")
    assert not planes[12].any() and np.isnan(normals).all()


@pytest.mark.gpu
def test_max_distance_knife_edge(hip):
    n, k = 500, 12
    pts, idx = family_cloud("volume", n, k)
    _, dist = R.knn(pts, k)
    edge = float(dist[17, 6])
    assert dist[17, 5] < edge < dist[17, 7]
    ref, (planes, _, _) = check(hip, pts, idx, max_distance=edge, what="the exact distance is in")
    assert planes[12][17] == 7
    ref, (planes, _, _) = check(hip, pts, idx, max_distance=float(np.nextafter(edge, 0.0)), what="one ulp below it is out")
    assert planes[12][17] == 6
    # 0.0 keeps only coincident points
    dup = pts.copy()
    dup[idx[40, 1:4]] = dup[40]
    didx, _ = R.knn(dup, k)
    ref, (planes, _, _) = check(hip, dup, didx, max_distance=0.0, what="zero")
    assert planes[12][40] == 4 and np.all(planes[0][planes[12] >= 3] == 0.0) and np.isnan(planes[3][40]) and (planes[12] == 1).sum() >= n - 8
    # a limit that leaves m = 2: the NaN
    two = float(dist[23, 1])
    ref, (planes, normals, _) = check(hip, pts, idx, max_distance=two, what="m = 2")
    assert planes[12][23] == 2 and np.isnan(planes[:12, 23]).all() and np.isnan(normals[23]).all()


@pytest.mark.gpu
def test_feature_selection(hip):
    """Every single bit, all thirteen, some sets in between: one plane per set bit in ascending bit order, and nothing else is written."""
    n, k = 300, 10
    pts, idx = family_cloud("plane_rotated", n, k)
    buf = TO.make_buffer(hip, pts, "H")
    ref = F.features(pts, idx)
    for features in [1 << t for t in range(13)] + [F.ALL, 8 | 16 | 32 | 512, 1 | 4096, 1024 | 2048, 2 | 64 | 128 | 256]:
        got = gpu_features(hip, pts, idx, features=features, buffer=buf)
        assert got[0].shape == (bin(features).count("1"), n)
        compare(got, ref, features, what=f"features={features}")
    # d_out NULL with only the normals asked for; and only the directions
    planes, normals, directions = gpu_features(hip, pts, idx, features=8, buffer=buf, out=False, directions=False)
    assert planes is None and directions is None
    compare((None, normals, None), ref)
    compare(gpu_features(hip, pts, idx, features=8, buffer=buf, out=False, normals=False), ref)
    # without the vectors nothing but the planes is written (the call would fault on a wild pointer otherwise)
    compare(gpu_features(hip, pts, idx, features=F.ALL, buffer=buf, normals=False, directions=False), ref)


@pytest.mark.gpu
def test_vector_orientation(hip):
    """Normals and directions are unit within 4 * 2^-52 and oriented by the rule; a vertical wall in the x-z plane has normals with an exact
    zero z (and x), and the lines and strips of an axis-aligned plane directions with one."""
    rng = np.random.default_rng(9)
    wall = np.column_stack([rng.random(400) * 30.0, np.full(400, 2.0), rng.random(400) * 10.0])
    floor = np.column_stack([rng.random(400) * 30.0, rng.random(400) * 30.0, np.full(400, 3.0)])
    zero_z = 0
    for name, pts in (("wall", wall), ("floor", floor), ("volume", F.family("volume", 400)[0]), ("line", F.family("line_rotated", 400)[0])):
        idx, _ = R.knn(pts, 10)
        ref, (_, normals, directions) = check(hip, pts, idx, what=name)
        for v in (normals, directions):
            assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 4 * 2.0 ** -52
            x, y, z = v[:, 0], v[:, 1], v[:, 2]
            assert not ((z < 0) | ((z == 0) & (y < 0)) | ((z == 0) & (y == 0) & (x < 0))).any()
            zero_z += int((z == 0).sum())
        if name == "wall":
            assert np.array_equal(bits(normals), bits(np.tile([0.0, 1.0, 0.0], (400, 1))))
        if name == "floor":
            assert np.all(directions[:, 2] == 0.0) and np.all(directions[:, 1] >= 0.0) and np.signbit(directions[:, 2]).any()  # negated ones carry -0.0
            assert np.all(normals[:, 2] == 1.0)
    assert zero_z >= 800


@pytest.mark.gpu
def test_storages_and_repeatability(hip):
    """VectorBuffer, HashMapBuffer, a slice and external memory at an odd byte offset give the same bytes; so do two calls."""
    n, k = 700, 16
    pts, idx = family_cloud("utm", n, k)
    ref = F.features(pts, idx)
    first = None
    for storage in ("H", "V", "sliceH", "sliceV", "packedV", "packedH", "external", "H"):
        got = gpu_features(hip, pts, idx, storage=storage)
        compare(got, ref, what=storage)
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert np.array_equal(bits(a), bits(b)), storage


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["volume", "surface"])
@pytest.mark.parametrize("n", [300, 5000])
def test_full_call(hip, shape, n):
    """pst_geometric_features (n = 300: the brute search, n = 5000: the grid search) is bit-identical to the from-lists entry fed with the lists
    it returned, and those lists' slot distances are the restatement's."""
    import torch
    k = 10
    pts = TO.cloud(n, 5, shape)
    buf = TO.make_buffer(hip, pts, "H")
    lists = torch.full((n, k), 7, dtype=torch.int32, device="cuda")
    out = torch.full((13, n), SENTINEL, dtype=torch.float64, device="cuda")
    nr = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    dr = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    alg.geometric_features_device(buf, k, F.ALL, out.data_ptr(), INF, nr.data_ptr(), dr.data_ptr(), lists.data_ptr())
    idx = lists.cpu().numpy().view(np.uint32).astype(np.int64)
    assert idx.max() < n and np.array_equal(idx[:, 0], np.arange(n))
    d = pts[idx] - pts[:, None, :]
    _, want = R.knn(pts, k)
    assert np.array_equal(bits(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])), bits(want))
    full = (out.cpu().numpy(), nr.cpu().numpy(), dr.cpu().numpy())
    again = gpu_features(hip, pts, idx, buffer=buf)
    for a, b in zip(full, again):
        assert np.array_equal(bits(a), bits(b))
    compare(full, F.features(pts, idx))
    # the same without the lists handed back, and through the dict interface (with and without a caller's lists)
    out2 = torch.full((13, n), SENTINEL, dtype=torch.float64, device="cuda")
    alg.geometric_features_device(buf, k, F.ALL, out2.data_ptr())
    assert np.array_equal(bits(out2.cpu().numpy()), bits(full[0]))
    r = alg.geometric_features(buf, k, return_normals=True, return_directions=True)
    assert list(r) == ["linearity", "planarity", "scattering", "verticality", "normals", "directions"]
    r2 = alg.geometric_features(buf, k, features=("verticality", "count", "linearity"), knn=idx, max_distance=float(np.median(want[:, 6])))
    ref2 = F.features(pts, idx, float(np.median(want[:, 6])))
    assert list(r2) == ["verticality", "count", "linearity"] and 3 < r2["count"].mean() < 10
    for name, t in (("linearity", 3), ("planarity", 4), ("scattering", 5), ("verticality", 9)):
        assert np.array_equal(bits(r[name]), bits(full[0][t])), name
    assert np.array_equal(bits(r["normals"]), bits(full[1])) and np.array_equal(bits(r["directions"]), bits(full[2]))
    for name in r2:
        assert np.array_equal(bits(r2[name]), bits(ref2[name])), name
    for bad_k, code in ((2, 12), (65, 23)):
        assert _code(lambda: alg.geometric_features(buf, bad_k)) == code
    assert _code(lambda: alg.geometric_features(TO.make_buffer(hip, pts[:2], "H"), 3)) == 11


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/pole_detection.py: the two poles come out as clusters, the boxes do not."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pole_detection", os.path.join(root, "examples", "pole_detection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(60_000)
    assert result["poles_found"] == result["poles_planted"] == 2 and result["box_points_kept"] == 0
