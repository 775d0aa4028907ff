"""Fixed-radius neighbour search without a GPU: the numpy restatement (tests/radius_ref.py) on hand-built cases, its bucketed-grid variant
against its brute force, the RadiusNeighbours helpers, the kernels' seams and every refusal the calls answer before a device is looked for,
through pa.radius_search and pa.radius_neighbour_counts and through the C entry points."""
import ctypes as C
import math

import numpy as np
import pytest

import pasture_amd as pa
import radius_ref as R
from pasture_amd import PastureError
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A

INF = float("inf")
NAN = float("nan")
IDENTITY = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(bits(a[2]), bits(b[2]))


def lattice(m=5):
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------------- the restatement

def both(query, target, radius, transform=None, edges=(None, 0.3, 7.0)):
    want = R.search(query, target, radius, transform)
    for edge in edges:
        assert same(R.search_grid(query, target, radius, edge, transform), want), edge
    return want


def test_restatement_empty_and_one_target():
    q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    off, idx, dist = both(q, np.zeros((0, 3)), 1.0)
    assert off.dtype == np.uint64 and idx.dtype == np.uint32 and dist.dtype == np.float64
    assert np.array_equal(off, [0, 0, 0, 0]) and idx.size == 0 and dist.size == 0
    off, idx, dist = both(np.zeros((0, 3)), q, 1.0)
    assert np.array_equal(off, [0]) and idx.size == 0
    # one target at the origin: the bound is inclusive, one ulp below it is not
    off, idx, dist = both(q, q[:1], 1.0)
    assert np.array_equal(off, [0, 1, 2, 2]) and np.array_equal(idx, [0, 0]) and np.array_equal(dist, [0.0, 1.0])
    off, idx, dist = both(q, q[:1], np.nextafter(1.0, 0.0))
    assert np.array_equal(off, [0, 1, 1, 1]) and np.array_equal(idx, [0])
    assert np.array_equal(R.counts(q, q[:1], 3.0), [1, 1, 1])


def test_restatement_coincident_points_are_listed_by_index():
    t = np.tile([[2.0, -1.0, 0.5]], (7, 1))
    off, idx, dist = both(t[:2], t, 0.25)
    assert np.array_equal(off, [0, 7, 14]) and np.array_equal(idx, list(range(7)) * 2) and not dist.any()


@pytest.mark.parametrize("r2,inner,face,corner", [(1, 7, 6, 4), (2, 19, 14, 7), (3, 27, 18, 8)])
def test_restatement_on_the_integer_lattice(r2, inner, face, corner):
    """5 x 5 x 5 unit lattice, self-search at radius^2 = 1, 2, 3: 6 neighbours at distance 1, 12 at sqrt(2), 8 at sqrt(3) and the point itself."""
    pts = lattice()
    radius = math.sqrt(r2)
    if radius * radius < r2:  # (sqrt(2)^2 rounds above 2, sqrt(3)^2 below 3: take the next double that includes the shell)
        radius = np.nextafter(radius, INF)
    off, idx, dist = both(pts, pts, radius, edges=(None, 0.7, 2.5))
    c = np.diff(off).reshape(5, 5, 5)
    assert c[2, 2, 2] == inner and c[0, 2, 2] == face and c[0, 0, 0] == corner
    first = idx[off[:-1].astype(np.int64)]
    assert np.array_equal(first, np.arange(125)) and not dist[off[:-1].astype(np.int64)].any()   # itself first, at distance 0
    a, b = int(off[62]), int(off[63])
    assert np.all(np.diff(dist[a:b]) >= 0)
    shell = idx[a + 1:a + 7]                                                                     # equal distances: ascending index
    assert np.array_equal(shell, np.sort(shell)) and np.array_equal(dist[a + 1:a + 7], np.ones(6))
    # one ulp below the shell loses exactly that shell
    below = R.counts(pts[62:63], pts, np.nextafter(math.sqrt(r2), 0.0) if math.sqrt(r2) ** 2 >= r2 else math.sqrt(r2))
    assert below[0] == {1: 1, 2: 7, 3: 19}[r2]


def test_restatement_non_finite_rows_and_transform():
    t = np.array([[0.0, 0.0, 0.0], [NAN, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, -0.5]])
    q = np.array([[0.0, 0.0, 0.0], [0.0, NAN, 0.0], [INF, 0.0, 0.0], [0.25, 0.0, 0.0]])
    off, idx, dist = both(q, t, 0.5)
    assert np.array_equal(off, [0, 3, 3, 3, 5])
    assert np.array_equal(idx, [0, 2, 4, 0, 2]) and np.array_equal(dist, [0.0, 0.5, 0.5, 0.25, 0.25])
    # a translation that puts query 3 onto target 2; one that overflows every query
    off, idx, dist = both(q, t, 0.1, [[1, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, 1, 0]])
    assert np.array_equal(off, [0, 0, 0, 0, 1]) and idx[0] == 2 and dist[0] == 0.0
    # a transform that overflows query 0 to +inf and puts query 1 onto the one target
    far = [[1e308, 0, 0, 1e308], [0, 1, 0, 0], [0, 0, 1, 0]]
    off, idx, dist = R.search([[2.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[1e308, 0.0, 0.0]], 1.0, far)
    assert np.array_equal(off, [0, 0, 1]) and idx[0] == 0 and dist[0] == 0.0


def test_bucketed_grid_equals_brute_force_on_random_clouds():
    rng = np.random.default_rng(3)
    t = rng.random((400, 3)) * [10.0, 10.0, 2.0]
    q = np.concatenate([rng.random((150, 3)) * [10.0, 10.0, 2.0], rng.random((30, 3)) * 30.0 - 10.0])
    for radius in (0.3, 1.1, 4.0):
        both(q, t, radius, edges=(None, radius / 3.1, radius * 5.0))


# ------------------------------------------------------------------------------------------------------------------- helpers and seams

def test_radius_neighbours_helpers():
    rn = pa.RadiusNeighbours(np.array([0, 3, 3, 4, 9], dtype=np.uint64), np.array([5, 1, 2, 7, 0, 1, 2, 3, 4], dtype=np.uint32),
                             np.array([0.0, 1.0, 2.0, 0.5, 0.0, 0.1, 0.2, 0.3, 0.4]))
    assert rn.counts.dtype == np.uint32 and np.array_equal(rn.counts, [3, 0, 1, 5])
    i, d = rn.list(3)
    assert np.array_equal(i, [0, 1, 2, 3, 4]) and np.array_equal(d, [0.0, 0.1, 0.2, 0.3, 0.4])
    assert rn.list(1)[0].size == 0
    p = rn.to_padded(4)
    N = 0xFFFFFFFF
    assert p.dtype == np.uint32 and np.array_equal(p, [[5, 1, 2, N], [N, N, N, N], [7, N, N, N], [0, 1, 2, 3]])
    assert rn.to_padded(0).shape == (4, 0)
    none = pa.RadiusNeighbours(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), None)
    assert none.to_padded(3).shape == (0, 3) and none.counts.size == 0
    assert pa.RadiusNeighbours(rn.offsets, rn.indices, None).list(0)[1] is None


def test_kernel_shape(hip):
    s = pa.radius_kernel_shape(hip)
    assert set(s) == {"queries_per_block", "sort_cap", "sort_window", "sort_positions_per_block"}
    assert s["sort_positions_per_block"] + s["sort_cap"] - 1 <= s["sort_window"] and s["sort_window"] & (s["sort_window"] - 1) == 0
    assert s["queries_per_block"] >= 64 and s["sort_cap"] >= 2
    one = C.c_uint32()
    hip.radius_kernel_shape(None, C.byref(one), None, None)  # each pointer is optional
    assert one.value == s["sort_cap"]
    hip.radius_kernel_shape(None, None, None, None)
    assert tuple(pa.radius_phase_times(hip)) == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(PastureError) as e:
        hip.radius_phase_times(None)
    assert e.value.code == 1


# ------------------------------------------------------------------------------------------------------------------- refusals on the host

def _empty_buffer(hip, dtype=T.Vec3f64):
    return HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _d(values):
    return (C.c_double * len(values))(*values)


class _BlankIndex:
    """A NearestNeighbourIndex over an empty target, stood up on the host (every field of pst_nn_index zero, as nn_index.hpp allows): for
    calls that are answered before the index is looked at.  It is never handed to pst_nn_index_destroy."""

    def __init__(self, hip):
        self.block = (C.c_uint8 * 4096)()
        self.index = object.__new__(alg.NearestNeighbourIndex)
        self.index.api = hip
        self.index._h = C.c_void_p(C.addressof(self.block))

    def __enter__(self):
        return self.index

    def __exit__(self, *exc):
        self.index._h = None


BAD_RADII = (NAN, INF, -INF, 0.0, -0.0, -1.0, 1e-160, 1e-170, 1e200)  # (1e-160)^2 is subnormal, (1e-170)^2 is zero, (1e200)^2 is +inf


def test_refusals_through_the_python_calls(hip):
    """A bad radius, a transform that is not finite, a query whose positions are not Vec3f64: the same status with or without a device,
    because none is looked for -- and the argument checks come before the attribute check."""
    buf, f32 = _empty_buffer(hip), _empty_buffer(hip, T.Vec3f32)
    with _BlankIndex(hip) as index:
        for call in (pa.radius_search, pa.radius_neighbour_counts):
            for radius in BAD_RADII:
                assert _code(lambda: call(buf, index, radius)) == 1, (call.__name__, radius)
                assert _code(lambda: call(f32, index, radius)) == 1
            for bad in (NAN, INF, -INF):
                for at in (0, 5, 11):
                    t = list(IDENTITY)
                    t[at] = bad
                    assert _code(lambda: call(buf, index, 1.0, transform=np.array(t).reshape(3, 4))) == 1
                    assert _code(lambda: call(f32, index, 1.0, transform=np.array(t).reshape(3, 4))) == 1
            assert _code(lambda: call(f32, index, 1.0)) == 4
            assert "Attribute not found" in str(pytest.raises(PastureError, call, f32, index, 1.0).value)
        assert _code(lambda: pa.radius_neighbour_counts(buf, index, NAN, device_counts_ptr=8)) == 1
        assert _code(lambda: pa.radius_search_device(buf, index, 0.0, 8, 8, 8, 4)) == 1
        assert _code(lambda: pa.radius_search_device(f32, index, 1.0, 8, 8, 0, 4)) == 4
        with pytest.raises(ValueError):
            pa.radius_search(buf, index, 1.0, transform=np.zeros((2, 2)))


def test_refusals_of_the_c_entry_points(hip):
    """NULL arguments, in the order the header documents: before the radius, the transform and the attribute."""
    buf, f32 = _empty_buffer(hip), _empty_buffer(hip, T.Vec3f32)
    fake = C.c_void_p(8)   # stands for an index / a device array: never dereferenced, every call below fails before that
    total = C.c_uint64(77)
    tot = C.byref(total)
    assert _code(lambda: hip.radius_neighbour_counts_device(None, buf._h, None, 1.0, fake, tot)) == 1
    assert _code(lambda: hip.radius_neighbour_counts_device(fake, None, None, 1.0, fake, tot)) == 1
    assert _code(lambda: hip.radius_neighbour_counts_device(fake, buf._h, None, 1.0, None, None)) == 1   # not both
    assert _code(lambda: hip.radius_neighbour_counts_device(fake, f32._h, None, 1.0, None, None)) == 1   # (before the attribute)
    assert _code(lambda: hip.radius_search_device(None, buf._h, None, 1.0, fake, fake, fake, 4, tot)) == 1
    assert _code(lambda: hip.radius_search_device(fake, None, None, 1.0, fake, fake, fake, 4, tot)) == 1
    assert _code(lambda: hip.radius_search_device(fake, buf._h, None, 1.0, None, fake, fake, 4, tot)) == 1     # offsets are required
    assert _code(lambda: hip.radius_search_device(fake, buf._h, None, 1.0, fake, fake, fake, 4, None)) == 1    # and the total
    assert _code(lambda: hip.radius_search_device(fake, buf._h, None, 1.0, fake, None, fake, 4, tot)) == 1     # no indices: capacity 0 only
    for radius in BAD_RADII:
        assert _code(lambda: hip.radius_neighbour_counts_device(fake, buf._h, None, radius, fake, tot)) == 1
        assert _code(lambda: hip.radius_search_device(fake, f32._h, None, radius, fake, None, None, 0, tot)) == 1
    t = list(IDENTITY)
    t[7] = NAN
    assert _code(lambda: hip.radius_search_device(fake, f32._h, _d(t), 1.0, fake, fake, None, 4, tot)) == 1
    assert _code(lambda: hip.radius_search_device(fake, f32._h, _d(IDENTITY), 1.0, fake, fake, None, 4, tot)) == 4
    assert _code(lambda: hip.radius_neighbour_counts_device(fake, f32._h, None, 1.0, None, tot)) == 4
    assert total.value == 77  # a refused call writes nothing


def test_no_cpu_fallback_without_device(hip):
    """Past the host-side checks the device is looked for, and without one the answer is PST_ERR_NO_DEVICE, never a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    buf = _empty_buffer(hip)
    with _BlankIndex(hip) as index:
        for call in (lambda: pa.radius_search(buf, index, 1.0), lambda: pa.radius_neighbour_counts(buf, index, 1.0)):
            with pytest.raises(PastureError) as e:
                call()
            assert e.value.code == 21 and "no CPU fallback" in str(e.value)
