"""Minimum-distance (Poisson-disk) subsampling (pst_poisson_disk_mask, pst_sample_priorities, pst_sample_kernel_shape) against tests/sample_ref.py.

CPU tests pin the priority keys, the restatement (by hand, by brute force, and its two forms against each other) and the argument checks
answered on the host.  GPU tests compare the HIP path with the restatement: masks with np.array_equal, no tolerance anywhere -- the kept set is
a function of the conflict predicate and the keys alone, and numpy evaluates the predicate with the same roundings."""
import ctypes as C

import numpy as np
import pytest

import sample_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_clusters import chain
from test_outliers import make_buffer

U64P = C.POINTER(C.c_uint64)
B = 256     # points_per_block, asserted against pst_sample_kernel_shape below: the parametrisations need it at collection time
SWEEPS = 2  # sweeps_per_launch
ORDERS = ("shuffled", "index")


def sheet(n, seed, conflicts_per_point, radius=1.0):
    """n points of a thin sheet (a fifth of the radius thick) whose density gives about that many conflicts per point at `radius`"""
    rng = np.random.default_rng(seed)
    side = radius * np.sqrt(max(n, 1) * np.pi / conflicts_per_point)
    return rng.random((n, 3)) * np.array([side, side, 0.2 * radius])


def gpu_mask(hip, pts, radius, seed=0, order="shuffled", storage="H", device=False):
    """(mask, kept, rounds) with the mask through host or device memory"""
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip, kind=HashMapBuffer if storage == "H" else VectorBuffer)
    if not device:
        mask, kept, rounds = alg.poisson_disk_mask(buf, radius, seed, order)
        assert mask.dtype == np.uint8 and mask.shape == (buf.len(),)
        return mask, kept, rounds
    import torch
    m = torch.full((max(buf.len(), 1),), 7, dtype=torch.uint8, device="cuda")
    none, kept, rounds = alg.poisson_disk_mask(buf, radius, seed, order, device_mask_ptr=m.data_ptr())
    assert none is None
    return m.cpu().numpy()[:buf.len()], kept, rounds


def assert_exact(got, want, what="", bound=None):
    mask, kept, rounds = got
    bad = np.flatnonzero(mask != want)
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} mask bytes differ, first at {bad[:6]}: {mask[bad[:6]]} vs {want[bad[:6]]}"
    assert kept == int(want.sum()), f"{what}: kept {kept} vs {int(want.sum())}"
    if bound is not None:
        assert (1 if bound else 0) <= rounds <= bound, f"{what}: {rounds} launches, the synchronous simulation needs {bound}"


def check(hip, pts, radius, seed=0, order="shuffled", storage="H", device=False, what="", brute=False):
    """One device call against the restatement, the launches against the synchronous bound; returns the mask"""
    keys = R.priorities(order, seed, len(pts))
    want = (R.greedy_mask_brute if brute else R.greedy_mask)(pts, radius, keys)
    got = gpu_mask(hip, pts, radius, seed, order, storage, device)
    assert_exact(got, want, f"{what} {order} seed {seed} {storage}", R.synchronous_rounds(pts, radius, keys))
    return got[0]


# ------------------------------------------------------------------------------------------------------------------- the keys and the restatement

def test_priorities_equal_the_restatement(hip):
    for order in ORDERS:
        for seed in (0, 1, 7, 0xDEADBEEF, 2 ** 64 - 1, 0x9E3779B97F4A7C15):
            for first, count in ((0, 1000), (2 ** 32 - 500, 1000), (2 ** 64 - 3, 6), (12345, 0), (0, 1)):
                got = alg.sample_priorities(order, seed, first, count, api=hip)
                assert got.dtype == np.uint64 and np.array_equal(got, R.priorities(order, seed, count, first)), (order, seed, first, count)
    # the finaliser itself, on the published test vector of splitmix64 with state 0 (first output) and on index order
    assert int(R.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert alg.sample_priorities("shuffled", 0, 0, 1, api=hip)[0] == 0xE220A8397B1DCDAF
    assert alg.sample_priorities("index", 99, 2 ** 32 - 1, 3, api=hip).tolist() == [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]  # the seed is ignored
    assert np.array_equal(alg.sample_priorities("shuffled", 5, 0, 64, api=hip), alg.sample_priorities("shuffled", 5 + 2 ** 64, 0, 64, api=hip))
    hip.sample_priorities(0, 1, 2, 0, None)  # count 0 writes nothing and needs no array


def test_shuffled_keys_are_distinct(hip):
    for seed, first in ((0, 0), (3, 2 ** 32 - 500000)):
        keys = alg.sample_priorities("shuffled", seed, first, 10 ** 6, api=hip)
        assert len(np.unique(keys)) == 10 ** 6
        assert np.array_equal(keys, R.priorities("shuffled", seed, 10 ** 6, first))


def test_restatement_on_three_collinear_points():
    """0, 0.6 and 1.2 on the x axis, radius 1: the middle point conflicts with both ends (0.36 <= 1), the ends do not (1.44 > 1).  Whoever comes
    first among the three decides: the middle one alone, or both ends."""
    P = np.array([[0.0, 0, 0], [0.6, 0, 0], [1.2, 0, 0]])
    for f in (R.greedy_mask, R.greedy_mask_brute):
        assert f(P, 1.0, [0, 1, 2]).tolist() == [1, 0, 1]   # index order: 0 kept, 1 rejected by 0, 2 kept
        assert f(P, 1.0, [2, 0, 1]).tolist() == [0, 1, 0]   # the middle point first: both ends rejected
        assert f(P, 1.0, [1, 2, 0]).tolist() == [1, 0, 1]   # point 2 first, then point 0 (1.44 > 1: kept), then the middle one
        assert f(P, 0.5, [0, 1, 2]).tolist() == [1, 1, 1]   # 0.36 > 0.25: nothing conflicts
        assert f(P, 0.6, [0, 1, 2]).tolist() == [1, 0, 1]   # exactly the radius apart: (0.6 * 0.6 <= 0.6 * 0.6) conflicts
        assert f(P, np.nextafter(0.6, 0.0), [0, 1, 2]).tolist() == [1, 1, 1]
    st, rounds, hist = R.synchronous_states(P, 1.0, [0, 1, 2])
    assert st.tolist() == [1, 2, 1] and rounds == 3 and hist == [2, 1, 0]  # a chain in key order decides one point per round
    st, rounds, hist = R.synchronous_states(P, 1.0, [2, 0, 1])
    assert st.tolist() == [2, 1, 2] and rounds == 2 and hist == [2, 0]
    assert R.synchronous_rounds(np.full((4, 3), np.nan), 1.0, [0, 1, 2, 3]) == 0 and R.synchronous_rounds(np.zeros((0, 3)), 1.0, []) == 0


def test_restatement_by_brute_force():
    """n = 2000: the kept points are pairwise free of conflicts, every finite unkept point conflicts with a kept one of smaller key; the dict
    form, the brute form and the synchronous simulation agree."""
    rng = np.random.default_rng(21)
    for conflicts_per_point, order, seed in ((2, "shuffled", 1), (10, "shuffled", 2), (10, "index", 0), (40, "shuffled", 3)):
        P = sheet(2000, 22 + conflicts_per_point, conflicts_per_point)
        P[rng.choice(2000, 30, replace=False), rng.integers(0, 3, 30)] = np.nan
        finite = np.isfinite(P).all(axis=1)
        keys = R.priorities(order, seed, 2000)
        mask = R.greedy_mask(P, 1.0, keys)
        d = P[:, None, :] - P[None, :, :]
        with np.errstate(invalid="ignore"):
            hit = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= 1.0
        np.fill_diagonal(hit, False)
        kept = mask == 1
        assert not mask[~finite].any() and 0 < kept.sum() < finite.sum()
        assert not hit[np.ix_(kept, kept)].any(), "two kept points conflict"
        smaller = keys[None, :] < keys[:, None]  # [i, j]: j has the smaller key
        covered = (hit & smaller & kept[None, :]).any(axis=1)
        assert np.array_equal(covered[finite], ~kept[finite]), "an unkept point without a kept conflict of smaller key, or a kept one with"
        assert np.array_equal(mask, R.greedy_mask_brute(P, 1.0, keys))
        state, rounds, hist = R.synchronous_states(P, 1.0, keys)
        assert np.array_equal(state == 1, kept) and np.array_equal(state == 0, ~finite) and rounds == len(hist) >= 2
        pairs = R.conflict_pairs(P, 1.0)
        assert len(pairs) == int(hit.sum()) and hit[pairs[:, 0], pairs[:, 1]].all()


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _error(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code, e.value.message


def test_kernel_shape(hip):
    assert alg.sample_kernel_shape(hip) == {"points_per_block": B, "sweeps_per_launch": SWEEPS}
    one = C.c_uint32(7)
    hip.sample_kernel_shape(None, C.byref(one))  # each pointer is optional
    assert one.value == SWEEPS
    hip.sample_kernel_shape(None, None)
    assert alg.sample_phase_times(hip) == (0.0, 0.0, 0.0)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    kept, rounds = C.c_uint64(), C.c_uint32()
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    k, r = C.byref(kept), C.byref(rounds)
    assert _error(lambda: hip.poisson_disk_mask(None, 1.0, 0, 0, fake, 1, k, r)) == (1, "buffer must not be NULL")
    assert _error(lambda: hip.poisson_disk_mask(buf._h, 1.0, 0, 0, None, 1, k, r)) == (1, "mask must not be NULL")
    assert _error(lambda: hip.poisson_disk_mask(buf._h, 1.0, 0, 0, fake, 1, None, r)) == (1, "kept must not be NULL")
    assert _error(lambda: hip.poisson_disk_mask(buf._h, 1.0, 0, 0, fake, 7, k, r)) == (1, "invalid mask memory kind")
    for order in (2, 3, 0xFFFFFFFF):
        assert _error(lambda: hip.poisson_disk_mask(buf._h, 1.0, order, 0, fake, 1, k, r)) == (1, "pst_poisson_disk_mask: order must be 0 (shuffled) or 1 (index order)")
    # 1e-160 and 1e200: finite and positive, but the square is subnormal / infinite
    for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-160, 1e200, 5e-324):
        assert _error(lambda: hip.poisson_disk_mask(buf._h, radius, 0, 0, fake, 1, k, r)) == \
            (1, "pst_poisson_disk_mask: radius must be finite and positive, and its square a normal number"), radius
    # the order of the checks: a null mask is reported before a bad radius, a bad radius before a position that is not Vec3f64
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _error(lambda: hip.poisson_disk_mask(f32._h, -1.0, 0, 0, None, 1, k, r))[1] == "mask must not be NULL"
    assert _error(lambda: hip.poisson_disk_mask(f32._h, -1.0, 0, 0, fake, 1, k, r))[0] == 1
    assert _error(lambda: hip.poisson_disk_mask(f32._h, 1.0, 0, 0, fake, 1, k, r)) == (4, "Attribute not found in PointLayout of buffer")
    with pytest.raises(PasturePanic):
        hip.poisson_disk_mask(f32._h, 1.0, 1, 0, fake, 1, k, None)
    assert _error(lambda: hip.sample_priorities(2, 0, 0, 4, (C.c_uint64 * 4)())) == (1, "pst_sample_priorities: order must be 0 (shuffled) or 1 (index order)")
    assert _error(lambda: hip.sample_priorities(0, 0, 0, 4, None)) == (1, "keys must not be NULL")
    assert _error(lambda: hip.sample_phase_times(None)) == (1, "ms must not be NULL")
    with pytest.raises(ValueError):
        alg.poisson_disk_mask(buf, 1.0, order="random")


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    kept, rounds = C.c_uint64(), C.c_uint32()
    mask = (C.c_uint8 * 8)()
    for buf in (_empty_buffer(hip), _empty_buffer(hip, kind=VectorBuffer)):
        for order in (0, 1):
            with pytest.raises(PastureError) as e:
                hip.poisson_disk_mask(buf._h, 1.0, order, 5, mask, 1, C.byref(kept), C.byref(rounds))
            assert e.value.code == 21 and "no CPU fallback" in str(e.value)
    with pytest.raises(PastureError) as e:
        alg.subsample_min_distance(_empty_buffer(hip), 1.0)
    assert e.value.code == 21


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

LENGTHS = sorted({0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, 10 * B + 7})


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("conflicts_per_point", [2, 10])
def test_lengths_around_the_seams(hip, conflicts_per_point, n):
    assert alg.sample_kernel_shape(hip) == {"points_per_block": B, "sweeps_per_launch": SWEEPS}
    pts = sheet(n, 30 + conflicts_per_point, conflicts_per_point) if n else np.zeros((0, 3))
    if n >= B - 1:
        mean = len(R.conflict_pairs(pts, 1.0)) / n
        assert 0.5 * conflicts_per_point < mean < 1.5 * conflicts_per_point, "the sheet is to have about that many conflicts per point"
    case = 0
    for order in ORDERS:
        for seed in (0, 0xC0FFEE):
            mask = check(hip, pts, 1.0, seed, order, storage="H" if case % 2 else "V", device=case % 4 >= 2, what=f"n {n}")
            if n >= B - 1:
                assert 0 < mask.sum() < n
            case += 1
    if n == 0:
        for device in (False, True):
            assert gpu_mask(hip, pts, 1.0, device=device)[1:] == (0, 0)


def knife_pairs(gap):
    """Three pairs, one along each axis, from 0 to `gap` on that axis (so the gap is exact) and at least ten units from each other"""
    pts = []
    for axis in range(3):
        a = np.full(3, 10.0 * axis)
        a[axis] = 0.0
        b = a.copy()
        b[axis] = gap
        pts += [a, b]
    return np.array(pts)


@pytest.mark.gpu
def test_predicate_knife_edge(hip):
    """radius 0.5: points exactly 0.5 apart conflict (d2 == r2 == 0.25), points the next double apart do not"""
    at, above = knife_pairs(0.5), knife_pairs(float(np.nextafter(0.5, 1.0)))
    assert np.all(at[1::2] - at[::2] == np.eye(3) * 0.5) and np.all(above[1::2] - above[::2] == np.eye(3) * np.nextafter(0.5, 1.0))  # the gaps are exact
    for device in (False, True):
        mask, kept, rounds = gpu_mask(hip, at, 0.5, order="index", device=device)
        assert mask.tolist() == [1, 0, 1, 0, 1, 0] and kept == 3 and 1 <= rounds <= 2  # (the synchronous simulation needs two)
        mask, kept, rounds = gpu_mask(hip, above, 0.5, order="index", device=device)
        assert mask.tolist() == [1] * 6 and kept == 6 and rounds == 1
    for seed in (1, 2, 3):
        keys = R.priorities("shuffled", seed, 6)
        want = np.zeros(6, dtype=np.uint8)
        for p in range(3):
            want[2 * p + (0 if keys[2 * p] < keys[2 * p + 1] else 1)] = 1  # the smaller key of every pair
        assert_exact(gpu_mask(hip, at, 0.5, seed), want, f"seed {seed}")
        assert np.array_equal(R.greedy_mask(at, 0.5, keys), want)
        assert gpu_mask(hip, above, 0.5, seed)[0].tolist() == [1] * 6


_CHAIN = {}


def chain_case(axis, variant):
    """(points, the radius at which the longest link of the chain conflicts exactly, the double below): computed once"""
    if (axis, variant) not in _CHAIN:
        pts = chain(axis, variant)
        x = np.sort(pts[:, axis])[-3000:]
        d = x[1:] - x[:-1]
        g2 = float(((d * d + 0.0) + 0.0).max())  # the predicate's own expression for the longest link
        r = float(np.sqrt(g2))
        while r * r < g2:
            r = float(np.nextafter(r, np.inf))
        while float(np.nextafter(r, 0.0)) * float(np.nextafter(r, 0.0)) >= g2:
            r = float(np.nextafter(r, 0.0))
        pts.setflags(write=False)
        _CHAIN[(axis, variant)] = (pts, r, float(np.nextafter(r, 0.0)))
    return _CHAIN[(axis, variant)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["generic", "at_minimum", "negative"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_grid_knife_edge(hip, axis, variant):
    """Links of a chain that are exactly `radius` long, all along the chain and so across many cell boundaries: a grid whose cell edge
    equalled the radius would put some of them two cells apart and the stencil would miss the conflict.  The reference here uses no grid."""
    pts, at, below = chain_case(axis, variant)
    keys = R.priorities("shuffled", 4, len(pts))
    want_at, want_below = R.greedy_mask_brute(pts, at, keys), R.greedy_mask_brute(pts, below, keys)
    assert want_below.sum() > want_at.sum(), "one double below, the longest links no longer conflict"
    assert_exact(gpu_mask(hip, pts, at, 4), want_at, "at the radius", R.synchronous_rounds(pts, at, keys))
    assert_exact(gpu_mask(hip, pts, below, 4), want_below, "one double below", R.synchronous_rounds(pts, below, keys))
    check(hip, pts, at, order="index", brute=True, what="index order")


@pytest.mark.gpu
def test_independence_from_the_grid(hip):
    """One far point moves the AABB (every cell boundary shifts): the mask of the original points does not change and the far point is kept.
    Two groups 10^4 apart at radius 10^-3 need 10^7 cells per axis, more than 2^21 - 1: the cell edge is doubled, the result stays exact."""
    pts = sheet(3 * B + 1, 41, 10)
    for order in ORDERS:
        alone = check(hip, pts, 1.0, 9, order, what="alone")
        for far in ([-777.7, -55.5, -3.3], [1e6, 2e6, 3e6], [pts[:, 0].min() - 0.5 * 1.001, 0.0, 0.0]):
            both = np.concatenate([pts, [far]])  # (the far point is the LAST index: the keys of the others are unchanged)
            mask = check(hip, both, 1.0, 9, order, what=f"with {far}")
            assert mask[-1] == 1 and np.array_equal(mask[:-1], alone)
    rng = np.random.default_rng(15)
    groups = np.concatenate([rng.random((2000, 3)) * 0.02, rng.random((2000, 3)) * 0.02 + 1e4])
    groups = groups[rng.permutation(len(groups))]
    mask = check(hip, groups, 1e-3, 5, what="two groups 10^4 apart", brute=True)
    assert 0 < mask.sum() < len(groups)


@pytest.mark.gpu
def test_degenerate_clouds(hip):
    rng = np.random.default_rng(51)
    # duplicates: 1000 copies of each of three positions -- the copy of smallest key of each position
    three = np.array([[0.0, 0, 0], [5.0, 0, 0], [0.0, 7.0, 1.0]])
    dup = np.repeat(three, 1000, axis=0)[rng.permutation(3000)]
    for order in ORDERS:
        mask = check(hip, dup, 1.0, 11, order, what="duplicates")
        keys = R.priorities(order, 11, 3000)
        want = [int(np.flatnonzero((dup == p).all(axis=1))[np.argmin(keys[(dup == p).all(axis=1)])]) for p in three]
        assert sorted(np.flatnonzero(mask).tolist()) == sorted(want)
    # 4096 points inside one radius (a cube of half the radius: its diagonal is 0.87 radii): exactly one kept, the smallest key
    ball = 100.0 + rng.random((4096, 3)) * 0.5
    for order, seed in (("shuffled", 1), ("shuffled", 2), ("index", 0)):
        mask, kept, rounds = gpu_mask(hip, ball, 1.0, seed, order)
        assert kept == 1 and mask.sum() == 1 and mask[np.argmin(R.priorities(order, seed, 4096))] == 1 and 1 <= rounds <= 2
    # all points farther apart than the radius: all kept, one round
    g = np.arange(16, dtype=np.float64) * 1.5
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(4096)]
    for order in ORDERS:
        mask, kept, rounds = gpu_mask(hip, lattice, 1.0, 3, order, storage="V")
        assert mask.all() and kept == 4096 and rounds == 1
    # planar (z constant), collinear (along a diagonal), and a dense cell next to sparse ones
    planar = sheet(5 * B + 3, 52, 10)
    planar[:, 2] = -4.25
    line = np.outer(rng.random(5 * B + 3) * 300.0, [1.0, -2.0, 0.5]) + np.array([3.0, 3.0, 3.0])
    dense = np.concatenate([sheet(2 * B, 53, 2), 20.0 + rng.random((1000, 3)) * np.array([1.0, 1.0, 0.2])])
    dense = dense[rng.permutation(len(dense))]
    for name, pts in (("planar", planar), ("collinear", line), ("dense cell", dense)):
        for order in ORDERS:
            mask = check(hip, pts, 1.0, 6, order, what=name)
            assert 0 < mask.sum() < len(pts)


@pytest.mark.gpu
def test_chain(hip):
    """2 B + 1 collinear points 0.6 radii apart in index order: every point conflicts with its two neighbours only, so index order keeps every
    other point -- and decides one point per synchronous round.  The same points with shuffled keys."""
    n = 2 * B + 1
    pts = np.zeros((n, 3))
    pts[:, 0] = np.arange(n) * 0.6
    want = (np.arange(n) % 2 == 0).astype(np.uint8)
    keys = R.priorities("index", 0, n)
    assert np.array_equal(R.greedy_mask(pts, 1.0, keys), want) and R.synchronous_rounds(pts, 1.0, keys) == n
    for device in (False, True):
        got = gpu_mask(hip, pts, 1.0, order="index", device=device)
        assert_exact(got, want, "index order", n)
    for seed in (0, 8):
        check(hip, pts, 1.0, seed, "shuffled", what="chain")


@pytest.mark.gpu
def test_non_finite_points(hip):
    pts = sheet(4000, 61, 10)
    rng = np.random.default_rng(62)
    bad = rng.choice(4000, 180, replace=False)
    k = 0
    for coord in range(3):
        for value in (np.nan, np.inf, -np.inf):
            pts[bad[k:k + 20], coord] = value
            k += 20
    good = np.isfinite(pts).all(axis=1)
    assert (~good).sum() == 180
    for order in ORDERS:
        keys = R.priorities(order, 13, 4000)
        want = np.zeros(4000, dtype=np.uint8)
        want[good] = R.greedy_mask(pts[good], 1.0, keys[good])  # the finite subset with ITS keys, mapped back
        assert np.array_equal(want, R.greedy_mask(pts, 1.0, keys)), "the restatement on the whole cloud"
        for storage, device in (("H", False), ("V", True)):
            got = gpu_mask(hip, pts, 1.0, 13, order, storage, device)
            assert_exact(got, want, f"non-finite {order}", R.synchronous_rounds(pts, 1.0, keys))
            assert not got[0][~good].any()
    # a cloud of nothing but such points: an all-zero mask and no round
    none = np.full((100, 3), np.nan)
    none[::3, 1] = np.inf
    none[1::3, 2] = -np.inf
    for device in (False, True):
        mask, kept, rounds = gpu_mask(hip, none, 1.0, device=device)
        assert not mask.any() and (kept, rounds) == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("storage", ["H", "V", "sliceH", "sliceV", "packedV", "packedH", "external"])
def test_storage(hip, storage, device):
    """Columnar, interleaved, a slice (the parent's other points must not be seen), interleaved records with Position3D at an odd byte offset,
    caller's memory; the mask to host and to device memory."""
    pts = sheet(3 * B + 1, 71, 10)
    check(hip, pts, 1.0, 17, "shuffled", storage, device, what=storage)
    check(hip, pts, 1.0, 0, "index", storage, device, what=storage)


@pytest.mark.gpu
def test_determinism_and_seeds(hip):
    pts = sheet(1 << 15, 81, 10)
    buf = make_buffer(hip, pts, "H")
    first = alg.poisson_disk_mask(buf, 1.0, 5)
    second = alg.poisson_disk_mask(buf, 1.0, 5)
    assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]
    masks = {5: first[0]}
    for seed in (6, 2 ** 63 + 1):
        masks[seed] = alg.poisson_disk_mask(buf, 1.0, seed)[0]
    for seed, mask in masks.items():
        assert np.array_equal(mask, R.greedy_mask(pts, 1.0, R.priorities("shuffled", seed, len(pts)))), seed
    assert not np.array_equal(masks[5], masks[6]) and not np.array_equal(masks[6], masks[2 ** 63 + 1])


_SHEET = {}


def larger_sheet():
    """The 2 * 10^5 points of the round simulation: uniform in 100 x 100 x 0.5"""
    if "pts" not in _SHEET:
        pts = np.random.default_rng(1).random((200000, 3)) * np.array([100.0, 100.0, 0.5])
        pts.setflags(write=False)
        _SHEET["pts"] = pts
    return _SHEET["pts"]


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0.3, 0.6])
def test_larger_sheet(hip, radius):
    pts = larger_sheet()
    n = len(pts)
    keys = R.priorities("shuffled", 7, n)
    want = R.greedy_mask(pts, radius, keys)
    state, bound, history = R.synchronous_states(pts, radius, keys)
    assert np.array_equal(state == 1, want == 1), "the synchronous simulation ends in the greedy states"
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY], api=hip)
    buf = HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    buf.set_attribute_range(A.INTENSITY, range(0, n), (np.arange(n) % 65521).astype(np.uint16))
    got = alg.poisson_disk_mask(buf, radius, 7)
    print(f"radius {radius}: kept {got[1]} of {n}, {got[2]} launches, synchronous rounds {bound}, undecided {history}")
    assert_exact(got, want, f"radius {radius}", bound)
    # the library's own calls: the thinned cloud clustered at tolerance = radius is all singletons ...
    thin, kept = alg.subsample_min_distance(buf, radius, 7)
    assert kept == got[1] == thin.len() and np.array_equal(thin.view_attribute(A.POSITION_3D), pts[want == 1])
    labels, sizes = alg.euclidean_clusters(thin, radius)
    assert len(sizes) == kept and (sizes == 1).all() and np.array_equal(np.sort(labels), np.arange(kept, dtype=np.uint32))
    # ... and every rejected point has a kept one within the radius: dist = sqrt(d2) of a d2 <= r2, compared squared, one ulp of slack on
    # that side only (the sqrt rounds once more, the header says of the clusters' predicate)
    rejected = buf.filter(HashMapBuffer, (want == 0).astype(np.uint8))
    idx, dist = alg.nearest_neighbours(rejected, thin)
    r2 = np.float64(radius) * np.float64(radius)
    assert rejected.len() == n - kept and (idx != alg.NO_MATCH).all() and (dist * dist <= np.nextafter(r2, np.inf)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [HashMapBuffer, VectorBuffer])
def test_subsample_carries_every_attribute(hip, kind):
    pts = sheet(5 * B + 3, 91, 10)
    n = len(pts)
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY, A.CLASSIFICATION, A.GPS_TIME], api=hip)
    buf = HashMapBuffer.new_from_layout(layout)
    buf.resize(n)
    columns = {A.POSITION_3D: pts, A.INTENSITY: (np.arange(n) * 7 % 65521).astype(np.uint16), A.CLASSIFICATION: (np.arange(n) % 251).astype(np.uint8),
               A.GPS_TIME: np.arange(n) * 0.125 + 1e5}
    for attribute, values in columns.items():
        buf.set_attribute_range(attribute, range(0, n), values)
    for order, seed in (("shuffled", 3), ("index", 0)):
        want = R.greedy_mask(pts, 1.0, R.priorities(order, seed, n)) == 1
        out, kept = alg.subsample_min_distance(buf, 1.0, seed, order, out_buffer_type=kind)
        assert isinstance(out, kind) and kept == out.len() == int(want.sum()) and 0 < kept < n
        for attribute, values in columns.items():
            assert np.array_equal(out.view_attribute(attribute), values[want]), attribute.name()
    assert alg.subsample_min_distance(_empty_buffer(hip), 1.0)[0].len() == 0


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/thin_then_align.py: the thinned scan is smaller, and the transform found on it brings the WHOLE scan closer to where it was
    taken than it was before, as the transform found on all points does."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("thin_then_align", os.path.join(root, "examples", "thin_then_align.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kept, displaced, whole, thinned = mod.main(40000, 0.5)
    assert 0 < kept < 40000 and whole[0] >= 1 and thinned[0] >= 1
    assert whole[3] < displaced and thinned[3] < displaced, (displaced, whole, thinned)
