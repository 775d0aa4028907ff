"""Polygon crop and overlay (pst_polygon_set_*, pst_points_in_polygons_device, pst_polygon_mask_device, pst_buffer_set_u8_from_ids_device,
pst_crop_kernel_shape) against tests/crop_ref.py, the numpy restatement that evaluates every edge of every polygon for every point.

CPU tests pin the restatement on hand-computed cases and the argument checks answered on the host.  GPU tests compare ids, mask and count of
both kernels with np.array_equal, no tolerance anywhere: the definition is seven f64 operations per point and edge, each rounded once, which
numpy evaluates with the same roundings.  The numpy reference is kept small: never more than 200 003 points, and at most 20 000 for sets of
more than 512 edges."""
import ctypes as C

import numpy as np
import pytest

import crop_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

FLAT_POINTS_PER_BLOCK = 1024  # asserted against pst_crop_kernel_shape below: the parametrisations need them at collection time
BANDED_POINTS_PER_BLOCK = 256
FLAT_MAX_EDGES = 1024
NO = R.NO_POLYGON
KERNELS = [("flat", 0), ("banded", 1), ("banded", 2), ("banded", 7), ("banded", 4096), ("banded", 0), ("auto", 0)]

HOLED = [[R.rectangle(0, 0, 9, 9), R.rectangle(2, 2, 7, 7, reverse=True), R.rectangle(4, 4, 5, 5)]]  # a hole, and an island inside the hole
BOWTIE = [np.array([[0.0, 0.0], [2.0, 2.0], [2.0, 0.0], [0.0, 2.0]])]
OVERLAP = [R.rectangle(2, 2, 6, 6), R.rectangle(0, 0, 4, 4), R.rectangle(3, -1, 5, 3)]
PENTAGON = [np.array([[0.0, 0.0], [4.0, 0.0], [6.0, 3.0], [4.0, 5.0], [0.0, 5.0]])]  # horizontal, vertical and slanted edges


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype), A.CLASSIFICATION], api=hip))


def cloud(n, seed, lo=(-1.0, -1.0), hi=(10.0, 10.0)):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.normal(0.0, 1.0, n)])


def ulps(v):
    v = np.float64(v)
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def as_points(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.column_stack([xy, np.zeros(len(xy))])


# ------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_kernel_shape(hip):
    assert alg.crop_kernel_shape(hip) == {"flat_points_per_block": FLAT_POINTS_PER_BLOCK, "banded_points_per_block": BANDED_POINTS_PER_BLOCK,
                                          "flat_max_edges": FLAT_MAX_EDGES}
    one = C.c_uint32(7)
    hip.crop_kernel_shape(None, None, C.byref(one))  # each pointer is optional
    assert one.value == FLAT_MAX_EDGES
    hip.crop_kernel_shape(None, None, None)
    assert alg.NO_POLYGON == NO


def test_unit_square_is_half_open():
    """left and bottom edges inside, right and top edges outside; so of the four vertices only (0, 0) is inside"""
    sq = [R.rectangle(0.0, 0.0, 1.0, 1.0)]
    pts = as_points([(0, 0), (1, 0), (1, 1), (0, 1),                    # the vertices
                     (0, 0.5), (0.5, 0), (1, 0.5), (0.5, 1),            # mid-edges: left, bottom, right, top
                     (0.5, 0.5), (-0.5, 0.5), (1.5, 0.5), (0.5, -0.5), (0.5, 1.5)])
    want = [0, NO, NO, NO, 0, 0, NO, NO, 0, NO, NO, NO, NO]
    for polygons in (sq, [sq[0][::-1].copy()], [np.roll(sq[0], 2, axis=0)]):  # either direction, any first vertex
        assert R.point_ids(pts, polygons).tolist() == want
    one = np.nextafter(1.0, 0.0)
    assert R.point_ids(as_points([(one, one), (one, 0.0), (0.0, one)]), sq).tolist() == [0, 0, 0]


def test_ray_through_vertices_on_an_integer_lattice():
    """A diamond and a zig-zag whose vertices lie on lattice rows: the ray of a lattice point passes through vertices, and each is counted
    once by the half-open rule in y."""
    diamond = [np.array([[3.0, 0.0], [6.0, 3.0], [3.0, 6.0], [0.0, 3.0]])]
    gx, gy = np.meshgrid(np.arange(-1.0, 8.0), np.arange(-1.0, 8.0))
    pts = as_points(np.column_stack([gx.ravel(), gy.ravel()]))
    x, y = pts[:, 0], pts[:, 1]
    # by hand: the diamond is x in [|y - 3|, 6 - |y - 3|) for 0 <= y < 6 -- half-open in x and in y, so of its vertices only (0, 3) is inside
    h = np.abs(y - 3.0)
    want = (y >= 0) & (y < 6) & (x >= h) & (x < 6 - h)
    assert np.array_equal(R.point_ids(pts, diamond) != NO, want)
    zigzag = [np.array([[0.0, 0.0], [2.0, 2.0], [4.0, 0.0], [6.0, 2.0], [8.0, 0.0], [8.0, 4.0], [0.0, 4.0]])]
    row2 = as_points([(x, 2.0) for x in range(-1, 10)])  # the ray along y = 2 touches the two peaks
    assert (R.point_ids(row2, zigzag) != NO).tolist() == [False] + [True] * 8 + [False, False]


def test_hole_island_bowtie_duplicate_vertex_and_spike():
    pts = as_points([(1, 1), (3, 3), (4.5, 4.5), (8, 8), (9.5, 1), (2, 2), (7, 7), (4, 4), (5, 5)])
    assert (R.point_ids(pts, HOLED) != NO).tolist() == [True, False, True, True, False, False, True, True, False]
    # the bow-tie crosses itself at (1, 1): the left and right triangles are inside, above and below the crossing is outside.  The crossing
    # itself has d == 0 on both diagonals and is strictly left of the right side alone: one crossing, inside
    pts = as_points([(0.25, 1.0), (1.75, 1.0), (1.0, 0.25), (1.0, 1.75), (1.0, 1.0)])
    assert (R.point_ids(pts, BOWTIE) != NO).tolist() == [True, True, False, False, True]
    grid = cloud(500, 1, (-1, -1), (3, 3))
    closed = [np.concatenate([BOWTIE[0], BOWTIE[0][:1]])]  # a repeated first vertex adds only a degenerate edge
    assert np.array_equal(R.point_ids(grid, closed), R.point_ids(grid, BOWTIE))
    assert len(R.entries_of(closed)[0]) == len(R.entries_of(BOWTIE)[0])
    # a horizontal spike (out and back along y = 2) changes nothing: both its edges are dropped
    plain = [np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [4.0, 4.0], [0.0, 4.0]])]
    spike = [np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [9.0, 2.0], [4.0, 2.0], [4.0, 4.0], [0.0, 4.0]])]
    along = np.concatenate([as_points([(x, 2.0) for x in np.arange(-1.0, 11.0, 0.5)]), cloud(300, 2, (-1, -1), (10, 5))])
    assert np.array_equal(R.point_ids(along, spike), R.point_ids(along, plain))
    assert (R.point_ids(as_points([(5.0, 2.0), (8.5, 2.0)]), spike) == NO).all()


def test_overlapping_polygons_and_non_finite_points():
    pts = as_points([(1, 1), (3, 3), (5, 5), (4.5, 0), (3.5, 2.5), (7, 7)])
    assert R.point_ids(pts, OVERLAP).tolist() == [1, 0, 0, 2, 0, NO]  # the smallest index wins
    nan, inf = np.nan, np.inf
    pts = np.array([[1, 1, nan], [1, 1, inf], [1, 1, -inf], [nan, 1, 0], [1, nan, 0], [inf, 1, 0], [-inf, 1, 0], [1, inf, 0], [1, -inf, 0], [nan, nan, nan]])
    ids = R.point_ids(pts, OVERLAP)
    assert ids.tolist() == [1, 1, 1] + [NO] * 7  # z is ignored; a point whose x or y is not finite is in no polygon
    mask, count = R.mask_of(ids, outside=True)
    assert mask.tolist() == [0, 0, 0] + [1] * 7 and count == 7  # the complement, byte for byte


def fan_points(tris, rim, centre, seed=3):
    """points on the spokes, 1e-9 beside them, on the rim's vertices, and a random cloud over the fan"""
    c = np.asarray(centre, dtype=np.float64)
    s = np.linspace(0.0, 1.0, 21)
    on = np.concatenate([c + s[:, None] * (v - c) for v in rim])
    beside = np.concatenate([on + [1e-9, 0.0], on - [1e-9, 0.0], on + [0.0, 1e-9], on - [0.0, 1e-9]])
    rng = np.random.default_rng(seed)
    rand = c + rng.uniform(-110.0, 110.0, (3000, 2))
    return as_points(np.concatenate([on, beside, rim, rand]))


def test_xor_identity_on_a_fan():
    """40 triangles around a UTM-sized centre, every other one running the other way round: the shared spokes evaluate the identical
    expression in both triangles, so the XOR of the triangles' containments IS the containment of the rim polygon, and every point inside
    falls in exactly one triangle."""
    centre = (7.0e5, 7.0e5)
    tris, rim = R.fan(40, centre)
    pts = fan_points(tris, rim, centre)
    each = np.array([R.contains(pts, t) for t in tris])
    outline = R.contains(pts, rim)
    assert np.array_equal(np.logical_xor.reduce(each, axis=0), outline)
    assert np.array_equal(each.sum(axis=0), outline.astype(np.int64))
    assert 0.3 < outline.mean() < 0.9
    assert np.array_equal(R.contains(pts, tris), outline)  # one polygon made of all the triangles as rings: the even-odd rule is that XOR


def test_grid_of_rectangles_against_searchsorted():
    """vertical edges have an exact sign, so every point goes to exactly the cell that comparisons against the grid lines give"""
    xs, ys = 5.0e5 + np.linspace(0.0, 10.0, 9) * 1.1, 5.0e6 + np.linspace(0.0, 7.0, 7) * 0.7
    rng = np.random.default_rng(4)
    pts = as_points(np.column_stack([rng.uniform(xs[0] - 1, xs[-1] + 1, 4000), rng.uniform(ys[0] - 1, ys[-1] + 1, 4000)]))
    lines = as_points([(x, y) for x in np.concatenate([ulps(v) for v in xs]) for y in np.concatenate([ulps(v) for v in ys])])
    pts = np.concatenate([pts, lines])
    assert np.array_equal(R.point_ids(pts, R.grid_rectangles(xs, ys)), R.grid_cell_ids(pts, xs, ys))


def test_argument_errors_answered_on_the_host(hip):
    """Every check of pst_polygon_set_create and of the query calls: the same answer with or without a device, because none is looked for."""
    sq = np.array([0, 0, 1, 0, 1, 1, 0, 1], dtype=np.float64)
    xy = sq.ctypes.data_as(C.POINTER(C.c_double))
    out = C.c_void_p()

    def create(xy=xy, offsets=(0, 4), n_rings=None, polygons=None, bands=0, kernel=0, out=C.byref(out)):
        off = (C.c_uint64 * len(offsets))(*offsets) if offsets is not None else None
        pol = (C.c_uint32 * len(polygons))(*polygons) if polygons is not None else None
        return lambda: hip.polygon_set_create(xy, off, len(offsets) - 1 if n_rings is None else n_rings, pol, bands, kernel, out)
    assert _code(create(xy=None)) == 1 and _code(create(offsets=None, n_rings=1)) == 1 and _code(create(out=None)) == 1
    assert _code(create(n_rings=0)) == 1
    assert _code(create(offsets=(1, 4))) == 1 and _code(create(offsets=(0, 2))) == 1 and _code(create(offsets=(0, 4, 3))) == 1
    assert _code(create(kernel=3)) == 1
    assert _code(create(polygons=(1,))) == 1
    two = np.concatenate([sq, sq + 2.0])
    xy2 = two.ctypes.data_as(C.POINTER(C.c_double))
    assert _code(create(xy=xy2, offsets=(0, 4, 8), polygons=(0, 2))) == 1
    for bad in (np.nan, np.inf, -np.inf):
        broken = sq.copy()
        broken[3] = bad
        assert _code(create(xy=broken.ctypes.data_as(C.POINTER(C.c_double)))) == 1
    # the limits, named in the message
    with pytest.raises(PastureError, match="2\\^24 vertices"):
        create(offsets=(0, (1 << 24) + 1))()
    with pytest.raises(PastureError, match="2\\^24 bands"):
        create(bands=(1 << 24) + 1)()
    zig = np.column_stack([np.arange(4098.0), np.arange(4098) % 2]).ravel().copy()
    with pytest.raises(PastureError, match="2\\^27 directory entries"):
        create(xy=zig.ctypes.data_as(C.POINTER(C.c_double)), offsets=(0, 4098), bands=32768)()
    with pytest.raises(PastureError, match=f"at most {FLAT_MAX_EDGES} entries"):
        create(xy=zig.ctypes.data_as(C.POINTER(C.c_double)), offsets=(0, 4098), kernel=1)()
    assert not out.value
    with pytest.raises(ValueError):
        alg.PolygonSet([], api=hip)
    with pytest.raises(ValueError):
        alg.PolygonSet([np.zeros((4, 3))], api=hip)
    with pytest.raises(KeyError):
        alg.PolygonSet(BOWTIE, kernel="fast", api=hip)
    # the query calls.  `fake` stands for a set and for device arrays: never dereferenced, every call below is answered before that
    fake, count = C.c_void_p(8), C.c_uint64(9)
    buf = _empty_buffer(hip)
    assert _code(lambda: hip.points_in_polygons_device(None, buf._h, fake)) == 1
    assert _code(lambda: hip.points_in_polygons_device(fake, None, fake)) == 1
    assert _code(lambda: hip.polygon_mask_device(None, buf._h, 0, fake, C.byref(count))) == 1
    assert _code(lambda: hip.polygon_mask_device(fake, None, 0, fake, C.byref(count))) == 1
    assert _code(lambda: hip.polygon_set_info(None, None, None, None)) == 1
    hip.polygon_set_destroy(None)
    f32 = _empty_buffer(hip, T.Vec3f32)  # a position that is not Vec3f64 is known from the layout alone
    assert _code(lambda: hip.points_in_polygons_device(fake, f32._h, fake)) == 4
    assert _code(lambda: hip.polygon_mask_device(fake, f32._h, 1, fake, None)) == 4
    with pytest.raises(PasturePanic):
        hip.polygon_mask_device(fake, f32._h, 1, fake, None)
    for kind in (HashMapBuffer, VectorBuffer):  # an empty buffer is answered on the host: nothing selected, nothing written
        empty = _empty_buffer(hip, kind=kind)
        count.value = 9
        hip.polygon_mask_device(fake, empty._h, 0, None, C.byref(count))
        assert count.value == 0
        hip.polygon_mask_device(fake, empty._h, 1, None, None)
        hip.points_in_polygons_device(fake, empty._h, None)
        count.value = 9
        hip.buffer_set_u8_from_ids_device(empty._h, b"Classification", None, None, 3, C.byref(count))
        assert count.value == 0
        assert _code(lambda: hip.buffer_set_u8_from_ids_device(empty._h, b"Intensity", fake, fake, 3, None)) == 4   # no such attribute
        assert _code(lambda: hip.buffer_set_u8_from_ids_device(empty._h, b"Position3D", fake, fake, 3, None)) == 4  # not a U8 attribute
        assert _code(lambda: hip.buffer_set_u8_from_ids_device(empty._h, None, fake, fake, 3, None)) == 1
    assert _code(lambda: hip.buffer_set_u8_from_ids_device(None, b"Classification", fake, fake, 3, None)) == 1


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PastureError) as e:
        alg.PolygonSet(BOWTIE, api=hip)
    assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# -------------------------------------------------------------------------------------------------------------------------------- GPU tests

def make_set(hip, polygons, kernel="auto", bands=0):
    return alg.PolygonSet(polygons, bands=bands, kernel=kernel, api=hip)


def gpu_query(hip, buf, ps, outside=False, device=False):
    """(ids, mask, count) through host arrays or through caller-owned device memory"""
    n = buf.len()
    if not device:
        ids = alg.points_in_polygons(buf, ps)
        mask, count = alg.polygon_mask(buf, ps, outside)
        assert ids.dtype == np.uint32 and ids.shape == (n,) and mask.dtype == np.uint8 and mask.shape == (n,)
        return ids, mask, count
    import torch
    d_ids = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    d_mask = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    assert alg.points_in_polygons(buf, ps, device_ids_ptr=d_ids.data_ptr()) is None
    none, count = alg.polygon_mask(buf, ps, outside, device_mask_ptr=d_mask.data_ptr())
    assert none is None
    hip.stream_synchronize()
    return d_ids.cpu().numpy().view(np.uint32)[:n], d_mask.cpu().numpy()[:n], count


def assert_same(got, want_ids, outside=False, what=""):
    ids, mask, count = got
    bad = np.flatnonzero(ids != want_ids)
    assert bad.size == 0, f"{what}: {bad.size} of {len(want_ids)} ids differ, first at {bad[:4]}: {ids[bad[:4]]} vs {want_ids[bad[:4]]}"
    want_mask, want_count = R.mask_of(want_ids, outside)
    assert np.array_equal(mask, want_mask), f"{what}: the mask is not (id != NO_POLYGON) != outside"
    assert count == want_count, f"{what}: count {count} vs {want_count}"


def check_all_kernels(hip, pts, polygons, want=None, kernels=KERNELS, storage="H", what=""):
    """the same cloud and set under every kernel and number of bands: all identical to the restatement (and so to each other)"""
    want = R.point_ids(pts, polygons) if want is None else want
    n_entries = len(R.entries_of(polygons)[0])
    buf = make_buffer(hip, pts, storage)
    for kernel, bands in kernels:
        if kernel == "flat" and n_entries > FLAT_MAX_EDGES:
            continue
        ps = make_set(hip, polygons, kernel, bands)
        info = ps.info
        assert info["entries"] == n_entries and info["polygons"] == len(polygons)
        assert info["kernel"] == (kernel if kernel != "auto" else ("flat" if n_entries <= FLAT_MAX_EDGES else "banded"))
        assert_same(gpu_query(hip, buf, ps), want, what=f"{what} {kernel} B={bands}")
        ps.destroy()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,tile", [("flat", FLAT_POINTS_PER_BLOCK), ("banded", BANDED_POINTS_PER_BLOCK)])
def test_point_counts_around_the_seams(hip, kernel, tile):
    ps = make_set(hip, HOLED + OVERLAP, kernel, 7 if kernel == "banded" else 0)
    for n in (1, 2, tile - 1, tile, tile + 1, 3 * tile + 5):
        pts = cloud(n, n)
        want = R.point_ids(pts, HOLED + OVERLAP)
        for outside in (False, True):
            assert_same(gpu_query(hip, make_buffer(hip, pts, "H"), ps, outside, device=outside), want, outside, f"{kernel} n={n}")
    ps.destroy()


@pytest.mark.gpu
def test_entry_counts_around_the_seams(hip):
    tri = [np.array([[0.0, 0.0], [8.0, 1.0], [3.0, 9.0]])]
    assert len(R.entries_of(tri)[0]) == 3
    check_all_kernels(hip, cloud(5000, 10), tri, what="3 entries")
    pts = cloud(20000, 11, (-1.2, -1.2), (1.2, 1.2))
    for n_entries in (FLAT_MAX_EDGES - 1, FLAT_MAX_EDGES, FLAT_MAX_EDGES + 1):
        polygons = [R.star(n_entries)]
        assert len(R.entries_of(polygons)[0]) == n_entries  # no edge of this star is horizontal
        want = check_all_kernels(hip, pts, polygons, kernels=[("flat", 0), ("banded", 0), ("auto", 0)], what=f"{n_entries} entries")
        assert 0.2 < (want != NO).mean() < 0.8
    # one entry more than the flat kernel takes: automatic mode is banded (checked above through info), forced flat is refused
    assert _code(lambda: make_set(hip, [R.star(FLAT_MAX_EDGES + 1)], "flat")) == 1
    # a set whose entries are all horizontal has none, and nothing is inside
    flat_line = [np.array([[0.0, 1.0], [5.0, 1.0], [9.0, 1.0]])]
    pts = np.concatenate([cloud(3000, 12), as_points([(x, 1.0) for x in np.arange(-1.0, 11.0, 0.5)])])
    want = check_all_kernels(hip, pts, flat_line, what="all horizontal")
    assert (want == NO).all()


@pytest.mark.gpu
def test_bands_and_kernels_agree(hip):
    polygons = HOLED + [R.star(64, (4.5, 4.5), 5.5, 2.0)] + OVERLAP
    check_all_kernels(hip, cloud(50000, 20), polygons, what="bands and kernels")


@pytest.mark.gpu
def test_knife_edges(hip):
    ring = PENTAGON[0]
    xy = []
    for vx, vy in ring:  # every vertex and one ulp to either side, in both coordinates
        xy += [(x, y) for x in ulps(vx) for y in ulps(vy)]
    for a, b in zip(ring, np.roll(ring, -1, axis=0)):  # points on the edges (the slanted ones at exactly representable spots) and beside them
        for s in (0.25, 0.5, 0.75):
            mx, my = a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1])
            xy += [(x, y) for x in ulps(mx) for y in ulps(my)]
    box = (0.0, 0.0, 6.0, 5.0)
    for bands in (2, 7, 4096):  # y exactly on a band boundary -- the first y of band k by the restated expression -- and the ys next to it
        d = R.directory(PENTAGON, bands)
        for k in np.unique(np.linspace(1, bands - 1, 40).astype(int)):
            y = np.float64(d["ymin"] + k / d["scale"])
            near = [y]
            for _ in range(3):
                near = [np.nextafter(near[0], -np.inf)] + near + [np.nextafter(near[-1], np.inf)]
            b = R.band_of(np.array(near), d["ymin"], d["scale"], bands)
            assert b[0] == k - 1 and b[-1] == k  # the boundary is among them
            xy += [(x, v) for x in (-0.5, 0.0, 1.0, 4.0, 5.0, 6.0, 6.5) for v in near]
    for x in ulps(box[0]) + ulps(box[2]) + [-3.0, 9.0, 2.0]:  # on each side of the box, beyond it on all four sides, exactly on it
        for y in ulps(box[1]) + ulps(box[3]) + [-3.0, 9.0, 2.5]:
            xy.append((x, y))
    pts = as_points(xy)
    want = check_all_kernels(hip, pts, PENTAGON, what="knife edges")
    assert 0.05 < (want != NO).mean() < 0.95
    # the same at UTM scale, where one ulp is 2^-30 .. 2^-29
    moved = [PENTAGON[0] + [5.0e5, 5.0e6]]
    far = as_points([(x, y) for vx, vy in moved[0] for x in ulps(vx) for y in ulps(vy)])
    check_all_kernels(hip, far, moved, what="knife edges, UTM")


@pytest.mark.gpu
def test_shapes(hip):
    pts = cloud(20000, 30)
    check_all_kernels(hip, pts, HOLED, what="hole and island")
    check_all_kernels(hip, cloud(20000, 31, (-1, -1), (3, 3)), BOWTIE, what="bow-tie")
    want = check_all_kernels(hip, pts, OVERLAP, what="overlapping")
    assert set(np.unique(want).tolist()) == {0, 1, 2, NO}
    big = [R.star(4096, (4.5, 4.5), 5.5, 2.5)]
    assert len(R.entries_of(big)[0]) == 4096
    check_all_kernels(hip, pts, big, kernels=[("banded", 1), ("banded", 7), ("banded", 4096), ("auto", 0)], what="star of 4096 vertices")
    want = check_all_kernels(hip, pts, [R.rectangle(1e7, 1e7, 1e7 + 1, 1e7 + 1)], what="a polygon far from every point")
    assert (want == NO).all()
    utm = [R.star(24, (5.0e5, 5.0e6), 250.0, 100.0), R.rectangle(5.0e5 - 10, 5.0e6 - 400, 5.0e5 + 10, 5.0e6 - 300)]
    want = check_all_kernels(hip, cloud(20000, 32, (5.0e5 - 300, 5.0e6 - 450), (5.0e5 + 300, 5.0e6 + 300)), utm, what="UTM")
    assert set(np.unique(want).tolist()) == {0, 1, NO}


@pytest.mark.gpu
def test_grid_rectangles_and_fan(hip):
    xs, ys = 5.0e5 + np.arange(33) * 1.1, 5.0e6 + np.arange(33) * 0.7
    rng = np.random.default_rng(40)
    pts = as_points(np.column_stack([rng.uniform(xs[0] - 1, xs[-1] + 1, 16000), rng.uniform(ys[0] - 1, ys[-1] + 1, 16000)]))
    lines = as_points([(x, y) for x in np.concatenate([ulps(v) for v in xs[::4]]) for y in np.concatenate([ulps(v) for v in ys[::4]])])
    pts = np.concatenate([pts, lines])
    rects = R.grid_rectangles(xs, ys)
    assert len(rects) == 1024
    want = R.grid_cell_ids(pts, xs, ys)  # (the restatement agrees with it on a smaller grid: test_grid_of_rectangles_against_searchsorted)
    check_all_kernels(hip, pts, rects, want=want, kernels=[("banded", 1), ("banded", 7), ("banded", 4096), ("auto", 0)], what="1024 rectangles")
    # the fan: on the device result, the triangles as 40 polygons, as the 40 rings of one polygon, and the rim polygon select the same points
    centre = (7.0e5, 7.0e5)
    tris, rim = R.fan(40, centre)
    pts = fan_points(tris, rim, centre)
    buf = make_buffer(hip, pts, "H")
    outline = R.contains(pts, rim)
    for kernel, bands in (("flat", 0), ("banded", 7), ("banded", 4096)):
        sets = [make_set(hip, p, kernel, bands) for p in (tris, [tris], [rim])]
        ids = [alg.points_in_polygons(buf, s) for s in sets]
        assert np.array_equal(ids[0] != NO, outline) and np.array_equal(ids[1] != NO, outline) and np.array_equal(ids[2] != NO, outline)
        assert np.array_equal(ids[0], R.point_ids(pts, tris))
        for s in sets:
            s.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "V", "packedV", "packedH", "external", "sliceV"])
def test_storages_and_non_finite_points(hip, storage):
    """`external` is a packed interleaved layout with the position at byte 1 of a 25-byte record: every coordinate is misaligned"""
    pts = cloud(3 * FLAT_POINTS_PER_BLOCK + 77, 50)
    rng = np.random.default_rng(51)
    for col, bad in ((0, np.nan), (1, np.inf), (0, -np.inf), (1, np.nan), (2, np.nan), (2, np.inf)):
        pts[rng.integers(0, len(pts), 40), col] = bad
    polygons = HOLED + OVERLAP
    want = R.point_ids(pts, polygons)
    assert (want[~np.isfinite(pts[:, :2]).all(axis=1)] == NO).all() and (want[~np.isfinite(pts[:, 2])] != NO).any()
    buf = make_buffer(hip, pts, storage)
    for kernel, bands in (("flat", 0), ("banded", 7)):
        ps = make_set(hip, polygons, kernel, bands)
        for outside in (False, True):
            for device in (False, True):
                assert_same(gpu_query(hip, buf, ps, outside, device), want, outside, f"{storage} {kernel} outside={outside} device={device}")
        ps.destroy()


@pytest.mark.gpu
def test_count_pointer_determinism_and_empty_buffer(hip):
    import torch
    pts = cloud(2 * FLAT_POINTS_PER_BLOCK + 3, 60)
    polygons = HOLED + OVERLAP
    want_mask, want_count = R.mask_of(R.point_ids(pts, polygons))
    buf = make_buffer(hip, pts, "H")
    for kernel in ("flat", "banded"):
        ps = make_set(hip, polygons, kernel)
        d = torch.full((len(pts),), 7, dtype=torch.uint8, device="cuda")
        hip.polygon_mask_device(ps._h, buf._h, 0, C.c_void_p(d.data_ptr()), None)  # without the pointer: stream-ordered, nothing read back
        hip.stream_synchronize()
        assert np.array_equal(d.cpu().numpy(), want_mask)
        count = C.c_uint64(9)
        hip.polygon_mask_device(ps._h, buf._h, 0, C.c_void_p(d.data_ptr()), C.byref(count))
        assert count.value == want_count and np.array_equal(d.cpu().numpy(), want_mask)
        first, second = gpu_query(hip, buf, ps), gpu_query(hip, buf, ps)  # two calls write the same bytes
        assert all(np.array_equal(a, b) for a, b in zip(first[:2], second[:2])) and first[2] == second[2] == want_count
        for kind in (HashMapBuffer, VectorBuffer):
            empty = _empty_buffer(hip, kind=kind)
            ids, mask, n = gpu_query(hip, empty, ps)
            assert ids.shape == (0,) and mask.shape == (0,) and n == 0
            out, n = alg.crop(empty, ps) if kind is HashMapBuffer else (empty, 0)
            assert out.len() == 0 and n == 0
            assert alg.overlay(empty, A.CLASSIFICATION, ps, [6, 6, 6, 6]) == 0
        assert _code(lambda: hip.polygon_mask_device(ps._h, buf._h, 0, None, None)) == 1
        assert _code(lambda: hip.points_in_polygons_device(ps._h, buf._h, None)) == 1
        ps.destroy()


def classified_buffer(hip, pts, kind):
    """Position3D, Classification (9 everywhere) and Intensity; "packed": interleaved, Classification first, so the position sits at byte 1"""
    n = len(pts)
    attrs = [A.POSITION_3D, A.CLASSIFICATION, A.INTENSITY]
    layout = PointLayout.from_attributes_packed([A.CLASSIFICATION, A.POSITION_3D, A.INTENSITY], 1, api=hip) if kind == "packed" else PointLayout.from_attributes(attrs, api=hip)
    buf = (HashMapBuffer if kind == "H" else VectorBuffer).new_from_layout(layout)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    buf.set_attribute_range(A.CLASSIFICATION, range(0, n), np.full(n, 9, dtype=np.uint8))
    buf.set_attribute_range(A.INTENSITY, range(0, n), (np.arange(n) % 65536).astype(np.uint16))
    return buf


@pytest.mark.gpu
def test_crop_equals_filter_with_the_restated_mask(hip):
    pts = cloud(3 * FLAT_POINTS_PER_BLOCK + 41, 70)
    pts[5, 0] = np.nan
    pts[6, 2] = np.inf
    polygons = HOLED + OVERLAP
    ids = R.point_ids(pts, polygons)
    buf = classified_buffer(hip, pts, "H")
    for outside in (False, True):
        mask, count = R.mask_of(ids, outside)
        want = buf.filter(HashMapBuffer, mask)
        for given in (polygons, make_set(hip, polygons, "banded", 7)):  # a PolygonSet, or anything PolygonSet accepts
            got, n = alg.crop(buf, given, outside, out_buffer_type=HashMapBuffer)
            assert n == count == got.len() == want.len()
            for a in (A.POSITION_3D, A.CLASSIFICATION, A.INTENSITY):  # every attribute, byte for byte
                assert got.view_attribute(a).tobytes() == want.view_attribute(a).tobytes(), (outside, a.name())
        got, n = alg.crop(buf, polygons, outside, out_buffer_type=VectorBuffer)
        assert n == count and np.array_equal(got.get_point_range(range(0, n)), buf.filter(VectorBuffer, mask).get_point_range(range(0, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["H", "V", "packed"])
def test_overlay(hip, kind):
    import torch
    pts = cloud(2 * FLAT_POINTS_PER_BLOCK + 9, 80)
    pts[3, 1] = np.nan
    polygons = OVERLAP + HOLED
    ids = R.point_ids(pts, polygons)
    values = np.array([6, 17, 6, 200], dtype=np.uint8)
    buf = classified_buffer(hip, pts, kind)
    before = buf.get_point_range(range(0, len(pts))).copy() if kind != "H" else None
    written = alg.overlay(buf, A.CLASSIFICATION, polygons, values)
    hit = ids != NO
    want = np.where(hit, values[np.minimum(ids, 3)], 9).astype(np.uint8)
    assert written == hit.sum() and np.array_equal(buf.view_attribute(A.CLASSIFICATION), want)
    assert np.array_equal(buf.view_attribute(A.POSITION_3D), pts, equal_nan=True)
    assert np.array_equal(buf.view_attribute(A.INTENSITY), (np.arange(len(pts)) % 65536).astype(np.uint16))
    if before is not None:  # interleaved: only the Classification byte of the points that were hit changed
        after = buf.get_point_range(range(0, len(pts)))
        assert ((after != before).sum(axis=1) <= 1).all() and ((after != before).any(axis=1) == (hit & (want != 9))).all()
    # fewer values than polygons: a point whose polygon has no value keeps its class
    buf = classified_buffer(hip, pts, kind)
    assert alg.overlay(buf, A.CLASSIFICATION, polygons, values[:2]) == (ids < 2).sum()
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), np.where(ids < 2, values[np.minimum(ids, 1)], 9).astype(np.uint8))
    # pst_buffer_set_u8_from_ids_device alone: ids at and beyond n_values, and NO_POLYGON
    n = len(pts)
    raw = (np.arange(n) % 7).astype(np.uint32)
    raw[::5] = NO
    raw[1::11] = 4
    raw[2::13] = 1 << 31
    d_ids = torch.from_numpy(raw.view(np.int32)).cuda()
    d_values = torch.from_numpy(np.array([1, 2, 3, 4], dtype=np.uint8)).cuda()
    buf = classified_buffer(hip, pts, kind)
    count = C.c_uint64(77)
    hip.buffer_set_u8_from_ids_device(buf._h, b"Classification", C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_values.data_ptr()), 4, C.byref(count))
    want = np.where(raw < 4, np.array([1, 2, 3, 4], dtype=np.uint8)[np.minimum(raw, 3)], 9).astype(np.uint8)
    assert count.value == (raw < 4).sum() and np.array_equal(buf.view_attribute(A.CLASSIFICATION), want)
    hip.buffer_set_u8_from_ids_device(buf._h, b"Classification", C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_values.data_ptr()), 0, C.byref(count))  # no value: nothing written
    assert count.value == 0 and np.array_equal(buf.view_attribute(A.CLASSIFICATION), want)
    hip.buffer_set_u8_from_ids_device(buf._h, b"Classification", C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_values.data_ptr()), 2, None)  # stream-ordered
    hip.stream_synchronize()
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), np.where(raw < 2, np.array([1, 2], dtype=np.uint8)[np.minimum(raw, 1)], want))


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(25, 20), (40, 30)])
def test_cross_check_against_the_raster(hip, cols, rows):
    """The cells of pmf_grid as rectangles: points_in_polygons gives every point the cell the raster puts it in, and the per-cell counts are
    rasterize's COUNT plane.  Coordinates are multiples of 2^-10 and the cell is 2^-1, so the raster's (x - x0) / cell and the grid lines
    x0 + i * cell are all exact.  500 rectangles run under the flat kernel, 1200 under the banded one."""
    n, cell = 200_003, 0.5
    rng = np.random.default_rng(90)
    pts = np.column_stack([rng.integers(0, int(cols * cell * 1024), n) / 1024.0 + 3.0, rng.integers(0, int(rows * cell * 1024), n) / 1024.0 - 7.0, rng.normal(0, 1, n)])
    pts[0, :2] = (3.0, -7.0)
    pts[1, :2] = (3.0 + cols * cell - 1 / 1024.0, -7.0 + rows * cell - 1 / 1024.0)
    buf = make_buffer(hip, pts, "H")
    grid = alg.pmf_grid(buf, cell)
    assert (grid["cols"], grid["rows"], grid["origin"]) == (cols, rows, (3.0, -7.0))
    xs, ys = grid["origin"][0] + np.arange(cols + 1) * cell, grid["origin"][1] + np.arange(rows + 1) * cell
    ps = make_set(hip, R.grid_rectangles(xs, ys))
    assert ps.info["kernel"] == ("flat" if 2 * cols * rows <= FLAT_MAX_EDGES else "banded")
    ids = alg.points_in_polygons(buf, ps)
    col, row = ((pts[:, 0] - grid["origin"][0]) / cell).astype(np.int64), ((pts[:, 1] - grid["origin"][1]) / cell).astype(np.int64)
    assert np.array_equal(ids, (row * cols + col).astype(np.uint32))
    raster = alg.rasterize(buf, cell, stats=("count",))
    assert np.array_equal(np.bincount(ids, minlength=cols * rows).reshape(rows, cols).astype(np.float64), raster.planes["count"])
    ps.destroy()


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/crop_polygon.py: the crop agrees with plain comparisons against the parcel's sides, inside and outside partition the cloud,
    the footprints' points become class 6 and the objects inside the parcel come out as clusters."""
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        spec = importlib.util.spec_from_file_location("crop_polygon", os.path.join(root, "examples", "crop_polygon.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        result = mod.main(60000)
    finally:
        sys.path.remove(os.path.join(root, "examples"))
    assert result["inside"] == result["expected_inside"] and result["differ"] == 0
    assert result["inside"] + result["outside"] > 60000 and 0 < result["building"] < result["inside"]
    assert result["clusters"] >= 4  # three boxes and one of the two poles stand inside the parcel
