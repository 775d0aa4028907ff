"""Rasterisation (pst_rasterize, pst_grid_fill_device, pst_raster_kernel_shape, pst_raster_phase_times) against tests/raster_ref.py.

CPU tests pin the restatement on hand-computed rasters, its chunk rule, and the argument checks answered on the host.  GPU tests compare the
HIP paths with the restatement BIT FOR BIT (u64 views: NaNs as bits, -0.0 apart from +0.0), no tolerance anywhere: counts, minima and maxima
do not depend on any order, the sums have the chunked order of the header, and numpy's float64 arithmetic rounds every operation once, as
the kernels do."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import raster_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

POINTS_PER_BLOCK = 1024  # asserted against pst_raster_kernel_shape below: the parametrisations need them at collection time
CHUNK = 256
TILE_COLS = 64
TILE_ROWS = 32
MAX_FILL = 16
SEAM_COUNTS = [1, POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 5]
ALL = R.STATS
ORDER_FREE = ("count", "min", "max")  # the atomic path
PATHS = {"atomic": ORDER_FREE, "sorted": ALL}
WIDE_SEED = 5


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def cloud(n, seed, cols=7.0, rows=5.0):
    """n points over cols x rows with heights of mixed sign and very different sizes, so that a sum shows its order"""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.random(n) * cols, rng.random(n) * rows, R.wide_values(n, seed + 1)])


def sized_cloud(cols, rows, seed):
    """about one point per cell (a third of the cells stay empty), and two corner points that pin the automatic grid to cols x rows"""
    pts = cloud(cols * rows, seed, cols - 0.5, rows - 0.5)
    pts = np.concatenate([pts, [[0.0, 0.0, 0.5], [cols - 0.5, rows - 0.5, -0.25]]])
    assert R.auto_grid(pts, 1.0)[2:] == (cols, rows)
    return pts


def gpu_rasterize(hip, pts, cell=1.0, stats=ALL, values=None, mask=None, origin=None, dim=None, storage="H", device_out=False, buf=None):
    """-> (planes by name, the Raster record); values and mask go through device memory, the planes through host or device memory"""
    import torch
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    buf = buf if buf is not None else make_buffer(hip, pts, storage)
    dv = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda() if values is not None else None
    dm = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda() if mask is not None else None
    kw = dict(values=dv.data_ptr() if dv is not None else None, device_mask_ptr=dm.data_ptr() if dm is not None else None, origin=origin, dim=dim)
    if not device_out:
        r = alg.rasterize(buf, cell, stats, **kw)
        return r.planes, r
    cols, rows = dim if dim is not None else R.auto_grid(pts, cell)[2:]
    names = [s for s in R.STATS if s in stats]
    d = torch.full((len(names), rows, cols), 123.0, dtype=torch.float64, device="cuda")
    r = alg.rasterize(buf, cell, stats, device_out_ptr=d.data_ptr(), **kw)
    assert r.planes == {}
    return dict(zip(names, d.cpu().numpy())), r


def assert_planes(got, want, stats, what=""):
    for s in stats:
        assert got[s].shape == want[s].shape, f"{what}: {s} is {got[s].shape}, not {want[s].shape}"
        bad = np.argwhere(R.bits(got[s]) != R.bits(want[s]))
        assert bad.size == 0, f"{what}: {len(bad)} cells of {s} differ, first at {bad[:3].tolist()}: {got[s][tuple(bad[0])]!r} vs {want[s][tuple(bad[0])]!r}"


def check(hip, pts, cell=1.0, stats=ALL, what="", **kw):
    want, members, grid = R.rasterize(pts, cell, stats, values=kw.get("values"), mask=kw.get("mask"), origin=kw.get("origin"), dim=kw.get("dim"))
    got, r = gpu_rasterize(hip, pts, cell, stats, **kw)
    assert (r.origin[0], r.origin[1], r.cols, r.rows) == grid and r.cell_size == cell, (what, r, grid)
    assert r.n_members == members, (what, r.n_members, members)
    assert_planes(got, want, stats, what)
    return got, r


# ------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_restatement_on_a_hand_computed_raster(hip):
    """3 columns x 2 rows of 1 m cells at the origin.  Cell (0, 0) holds 1 and 3, cell (0, 1) a -0.0 / +0.0 pair, cell (1, 2) one 7; the other
    three are empty; a point on the right edge, one with a NaN height and one with an infinite x are no members."""
    pts = np.array([[0.5, 0.5, 1.0], [1.5, 0.5, -0.0], [0.2, 0.9, 3.0], [2.5, 1.5, 7.0], [1.6, 0.1, 0.0], [3.0, 0.5, 9.0], [0.5, 0.5, np.nan], [np.inf, 0.5, 1.0]])
    got, members, grid = R.rasterize(pts, 1.0, origin=(0.0, 0.0), dim=(3, 2))
    assert members == 5 and grid == (0.0, 0.0, 3, 2)
    nan = R.NAN
    expect = {"count": [[2.0, 2.0, 0.0], [0.0, 0.0, 1.0]], "min": [[1.0, -0.0, nan], [nan, nan, 7.0]], "max": [[3.0, 0.0, nan], [nan, nan, 7.0]],
              "mean": [[2.0, 0.0, nan], [nan, nan, 7.0]], "variance": [[1.0, 0.0, nan], [nan, nan, 0.0]]}
    assert_planes(got, {s: np.array(v) for s, v in expect.items()}, ALL)
    assert R.bits(got["min"])[0, 1] == 0x8000000000000000 and R.bits(got["max"])[0, 1] == 0  # -0.0 is below +0.0, and both keep their bits
    assert (R.bits(got["mean"])[0, 2], R.bits(got["count"])[0, 2]) == (0x7FF8000000000000, 0)  # an empty cell: the canonical NaN, count +0.0
    # the other order of the pair: the same extremes
    again = R.rasterize(pts[::-1], 1.0, origin=(0.0, 0.0), dim=(3, 2))[0]
    assert_planes(again, got, ORDER_FREE)
    # the automatic grid covers the points with three finite components: the NaN height and the infinite x take no part
    assert R.auto_grid(pts, 1.0) == (0.2, 0.1, 3, 2) and R.auto_grid(pts[6:], 1.0) == (0.0, 0.0, 0, 0)


def test_restatement_chunk_rule():
    """One cell of 2 * 256 + 1 values over 30 decades with mixed signs: the chunked sum is neither the plain left-to-right sum nor the sum of
    the reversed order, so these inputs tell the orders apart (the GPU tests below use them)."""
    v = R.wide_values(2 * CHUNK + 1, WIDE_SEED)
    assert np.log10(np.abs(v).max() / np.abs(v).min()) > 29 and (v > 0).any() and (v < 0).any()
    chunked = R.chunked_sum(v)
    by_hand = (R.plain_sum(v[:CHUNK]) + R.plain_sum(v[CHUNK:2 * CHUNK])) + v[2 * CHUNK]
    assert R.bits(chunked) == R.bits(by_hand)
    assert R.bits(chunked) != R.bits(R.plain_sum(v)) and R.bits(chunked) != R.bits(R.plain_sum(v[::-1])) and R.bits(chunked) != R.bits(R.chunked_sum(v[::-1]))
    assert R.bits(R.chunked_sum(v[:CHUNK])) == R.bits(R.plain_sum(v[:CHUNK]))  # one chunk: the plain sum
    pts = np.column_stack([np.full(len(v), 0.5), np.full(len(v), 0.5), v])
    got = R.rasterize(pts, 1.0)[0]
    assert R.bits(got["mean"])[0, 0] == R.bits(chunked / np.float64(len(v)))


def test_restatement_of_the_fill():
    nan, inf = R.NAN, np.inf
    a = np.array([[nan, 2.0, nan, nan, nan],
                  [4.0, inf, nan, nan, nan],
                  [nan, nan, nan, nan, 9.0]])
    got = R.fill(a, 1)
    want = np.array([[3.0, 2.0, 2.0, nan, nan],   # the corner: (2 + 4) / 2, the +inf entry next to it is empty; (0, 3) has no entry in reach
                     [4.0, 3.0, 2.0, 9.0, 9.0],   # the +inf entry is filled from its two neighbours; (1, 2) sees only the diagonal 2
                     [4.0, 4.0, nan, 9.0, 9.0]])
    assert np.array_equal(R.bits(got), R.bits(want))
    assert R.bits(got)[0, 3] == 0x7FF8000000000000
    # different weights, in row-major order: ((1 * 1 + 1 * 2) + 0.5 * 5) / ((1 + 1) + 0.5)
    assert R.fill(np.array([[nan, 1.0], [2.0, 5.0]]), 1)[0, 0] == ((1.0 + 2.0) + 0.5 * 5.0) / ((1.0 + 1.0) + 0.5)
    # the first visited cell SETS the sums: a lone -0.0 neighbour stays -0.0 (0.0 + -0.0 would be +0.0)
    assert R.bits(R.fill(np.array([[nan, -0.0]]), 1))[0, 0] == 0x8000000000000000
    assert np.array_equal(R.bits(R.fill(a, 0)), R.bits(a))  # h = 0: a copy
    assert np.isnan(R.fill(np.full((3, 4), nan), 2)).all()
    assert np.array_equal(R.fill(a, 4)[1], R.fill(a, 16)[1])  # every cell in reach already


def test_kernel_shape(hip):
    assert alg.raster_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK, "chunk": CHUNK, "fill_tile_cols": TILE_COLS, "fill_tile_rows": TILE_ROWS,
                                            "fill_max_half_width": MAX_FILL}
    assert R.CHUNK == CHUNK
    one = C.c_uint32(7)
    hip.raster_kernel_shape(None, None, None, None, C.byref(one))  # each pointer is optional
    assert one.value == MAX_FILL
    hip.raster_kernel_shape(None, None, None, None, None)
    assert alg.raster_phase_times(hip) == (0.0, 0.0, 0.0)
    assert _code(lambda: hip.raster_phase_times(None)) == 1


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments, invalid parameters, a missing position and an empty buffer with the automatic grid: the same answer with or without a
    device, because no device is looked for."""
    buf = _empty_buffer(hip)
    out, members = (C.c_double * 8)(*([5.0] * 8)), C.c_uint64(9)
    origin, dim = (C.c_double * 2)(0.0, 0.0), (C.c_uint32 * 2)(2, 2)
    nan, inf = float("nan"), float("inf")

    def call(b=buf._h, cell=1.0, o=None, d=None, stats=4, dst=out, kind=1, m=C.byref(members)):
        return lambda: hip.rasterize(b, None, None, cell, o, d, stats, dst, kind, None, None, m)
    assert _code(call(b=None)) == 1 and _code(call(dst=None)) == 1 and _code(call(m=None)) == 1
    assert _code(call(kind=7)) == 1  # no such memory kind
    for cell in (0.0, -1.0, nan, inf, -inf):
        assert _code(call(cell=cell)) == 1, cell
    for stats in (0, 32, 33, 1 << 31):
        assert _code(call(stats=stats)) == 1, stats
    assert _code(call(o=origin)) == 1 and _code(call(d=dim)) == 1  # one without the other
    for bad in ((0, 2), (2, 0), (0, 0)):
        assert _code(call(o=origin, d=(C.c_uint32 * 2)(*bad))) == 1, bad
    for bad in ((nan, 0.0), (0.0, inf)):
        assert _code(call(o=(C.c_double * 2)(*bad), d=dim)) == 1, bad
    assert _code(call(o=origin, d=(C.c_uint32 * 2)(1 << 15, (1 << 13) + 1))) == 23  # more than 2^28 cells
    with pytest.raises(ValueError):
        alg.rasterize(buf, 1.0, ("median",))
    with pytest.raises(ValueError):
        alg.rasterize(buf, 1.0, origin=(0.0, 0.0))
    with pytest.raises(ValueError):
        alg.rasterize(buf, 1.0, ("stdev",), device_out_ptr=8)
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(call(b=f32._h)) == 4 and _code(call(b=f32._h, o=origin, d=dim)) == 4
    with pytest.raises(PasturePanic):
        call(b=f32._h)()
    # an empty buffer with the automatic grid is answered on the host: a zero geometry, nothing written
    for kind in (HashMapBuffer, VectorBuffer):
        empty = _empty_buffer(hip, kind=kind)
        members.value = 9
        origin_out, dim_out = (C.c_double * 2)(3.0, 3.0), (C.c_uint32 * 2)(3, 3)
        hip.rasterize(empty._h, None, None, 1.0, None, None, 31, out, 1, origin_out, dim_out, C.byref(members))
        assert (members.value, tuple(origin_out), tuple(dim_out), list(out)) == (0, (0.0, 0.0), (0, 0), [5.0] * 8)
        r = alg.rasterize(empty, 1.0, ("count", "stdev"))
        assert (r.origin, r.cols, r.rows, r.n_members) == ((0.0, 0.0), 0, 0, 0) and r.planes["count"].shape == (0, 0) and r.planes["stdev"].shape == (0, 0)
    # the fill: a half-width beyond the tile, null rasters, in place, too many cells; a raster without cells is answered on the host
    fake, other = C.c_void_p(8), C.c_void_p(4096)  # never dereferenced: every call below fails before that
    assert _code(lambda: hip.grid_fill_device(fake, other, 4, 4, MAX_FILL + 1)) == 1
    assert _code(lambda: hip.grid_fill_device(None, other, 4, 4, 1)) == 1 and _code(lambda: hip.grid_fill_device(fake, None, 4, 4, 1)) == 1
    assert _code(lambda: hip.grid_fill_device(fake, fake, 4, 4, 1)) == 1
    assert _code(lambda: hip.grid_fill_device(fake, other, 1 << 15, (1 << 13) + 1, 1)) == 23
    hip.grid_fill_device(None, None, 0, 4, 1)
    hip.grid_fill_device(None, None, 4, 0, 0)
    assert _code(lambda: hip.grid_fill_device(None, None, 0, 4, MAX_FILL + 1)) == 1


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PastureError) as e:
        hip.grid_fill_device(C.c_void_p(8), C.c_void_p(4096), 4, 4, 1)
    assert e.value.code == 21 and "no CPU fallback" in str(e.value)
    # a caller's grid over an empty buffer still has planes to fill, and that needs the device
    out, members = (C.c_double * 4)(), C.c_uint64()
    empty = _empty_buffer(hip)
    assert _code(lambda: hip.rasterize(empty._h, None, None, 1.0, (C.c_double * 2)(0.0, 0.0), (C.c_uint32 * 2)(2, 2), 1, out, 1, None, None, C.byref(members))) == 21


# -------------------------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_point_counts_around_the_block(hip, n, path):
    check(hip, cloud(n, 100 + n), 1.0, PATHS[path], what=f"n={n} {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(1, 1), (1, 150), (150, 1), (TILE_COLS - 1, TILE_ROWS - 1), (TILE_COLS, TILE_ROWS), (TILE_COLS + 1, TILE_ROWS + 1),
                                       (2 * TILE_COLS + 1, TILE_ROWS + 1)])
def test_raster_sizes(hip, cols, rows):
    pts = sized_cloud(cols, rows, 7 * cols + rows)
    for path, stats in PATHS.items():
        got, r = check(hip, pts, 1.0, stats, what=f"{cols}x{rows} {path}")
        assert (r.cols, r.rows) == (cols, rows)
    # ... and the fill of that raster across the tile's edges
    want = R.fill(got["mean"], 2)
    assert np.array_equal(R.bits(gpu_fill(got["mean"], 2)), R.bits(want))


@pytest.mark.gpu
def test_both_paths_agree(hip):
    pts = cloud(3 * POINTS_PER_BLOCK + 5, 3)
    a, ra = gpu_rasterize(hip, pts, 0.5, ORDER_FREE)
    b, rb = gpu_rasterize(hip, pts, 0.5, ORDER_FREE + ("mean",))
    assert ra.n_members == rb.n_members == len(pts) and (ra.cols, ra.rows) == (rb.cols, rb.rows)
    for s in ORDER_FREE:
        assert a[s].tobytes() == b[s].tobytes(), s


def seam_cloud(counts, seed):
    """cell c of a 1-row raster holds counts[c] of the wide-range values; the points of all cells are interleaved at random"""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(col)
    v = R.wide_values(len(col), WIDE_SEED)
    return np.column_stack([col + rng.random(len(col)), rng.random(len(col)), v])


@pytest.mark.gpu
def test_chunk_seams(hip):
    counts = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1]
    pts = seam_cloud(counts, 21)
    got, r = check(hip, pts, 1.0, ALL, origin=(0.0, 0.0), dim=(len(counts), 1), what="seams")
    assert got["count"][0].tolist() == [float(c) for c in counts]
    # the inputs of test_restatement_chunk_rule in one cell: the mean is the chunked one, not the plain one
    v = R.wide_values(2 * CHUNK + 1, WIDE_SEED)
    one = np.column_stack([np.full(len(v), 0.5), np.full(len(v), 0.5), v])
    got, _ = check(hip, one, 1.0, ALL, what="one cell")
    assert R.bits(got["mean"])[0, 0] == R.bits(R.chunked_sum(v) / np.float64(len(v))) != R.bits(R.plain_sum(v) / np.float64(len(v)))


@pytest.mark.gpu
def test_a_dense_cell_next_to_a_sparse_one(hip):
    """40 * 256 + 3 members in descending order in one cell, every other point of the buffer in a second cell: the dense cell is summed by a
    workgroup, chunk by chunk, in buffer order."""
    m = 40 * CHUNK + 3
    v = np.sort(R.wide_values(m, 9))[::-1]
    pts = np.zeros((2 * m, 3))
    pts[0::2] = np.column_stack([np.full(m, 0.25), np.full(m, 0.5), v])
    pts[1::2] = np.column_stack([np.full(m, 1.75), np.full(m, 0.5), R.wide_values(m, 10)])
    for stats in (ALL, ("variance",), ("mean", "count")):
        got, r = check(hip, pts, 1.0, stats, origin=(0.0, 0.0), dim=(2, 1), what=f"dense {stats}")
    assert r.n_members == 2 * m


@pytest.mark.gpu
def test_order_of_the_points(hip):
    pts = seam_cloud([40, 300, 700], 33)
    perm = np.random.default_rng(4).permutation(len(pts))
    a, _ = check(hip, pts, 1.0, ALL, origin=(0.0, 0.0), dim=(3, 1), what="order a")
    b, _ = check(hip, pts[perm], 1.0, ALL, origin=(0.0, 0.0), dim=(3, 1), what="order b")
    for s in ORDER_FREE:
        assert a[s].tobytes() == b[s].tobytes(), s
    assert (R.bits(a["mean"]) != R.bits(b["mean"])).any()  # (both equal the restatement: it says the order shows)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_given_geometry_crops(hip, path):
    x0, y0, cell, cols, rows = 1.0, -2.0, 0.25, 4, 2  # x in [1, 2), y in [-2, -1.5)
    below, above = lambda v: np.nextafter(v, -np.inf), lambda v: np.nextafter(v, np.inf)
    xs = [x0, below(x0), above(x0), x0 + cols * cell, below(x0 + cols * cell), 1.25, below(1.25), above(1.25), 1.6, -7.0, 50.0]
    ys = [y0, below(y0), above(y0), y0 + rows * cell, below(y0 + rows * cell), -1.75, below(-1.75), above(-1.75)]
    pts = np.array([[x, y, 10.0 * i + j] for i, x in enumerate(xs) for j, y in enumerate(ys)])
    got, r = check(hip, pts, cell, PATHS[path], origin=(x0, y0), dim=(cols, rows), what=path)
    xin = [x for x in xs if x0 <= x < x0 + cols * cell]
    yin = [y for y in ys if y0 <= y < y0 + rows * cell]
    assert (len(xin), len(yin)) == (7, 6) and r.n_members == 42 == int(got["count"].sum())
    # columns: [1, 1.25) holds x0, the ulp above it and the ulp below 1.25; [1.25, 1.5) holds 1.25 and the ulp above; 1.6; the ulp below 2
    assert got["count"].sum(axis=0).tolist() == [18.0, 12.0, 6.0, 6.0] and got["count"].sum(axis=1).tolist() == [21.0, 21.0]
    assert (r.origin, r.cols, r.rows) == ((x0, y0), cols, rows)


@pytest.mark.gpu
def test_automatic_geometry_is_the_ground_filters(hip):
    pts = cloud(2500, 8, 40.0, 23.0)
    pts[::97, 2] = np.nan     # not finite: takes no part in either grid
    pts[5::101, 0] = np.inf
    mask = (np.arange(len(pts)) % 3 != 0).astype(np.uint8)
    buf = make_buffer(hip, pts, "H")
    grid = alg.pmf_grid(buf, 1.5)
    for m in (None, mask):  # the mask does not move the grid
        got, r = gpu_rasterize(hip, pts, 1.5, ("min", "count"), mask=m, buf=buf)
        assert (r.origin, r.cols, r.rows) == (grid["origin"], grid["cols"], grid["rows"])
    got, r = check(hip, pts, 1.5, ("min", "count"), buf=buf, what="auto")
    assert r.n_members == grid["n_finite"]
    z0 = alg.ground_mask(buf, alg.PmfParameters(1.5, 4.0, 1.0, 0.5, 3.0), return_surfaces=True)[2]["min_z"]
    full = np.isfinite(z0)
    assert np.array_equal(R.bits(got["min"][full]), R.bits(z0[full])) and (R.bits(got["min"][~full]) == R.NAN_BITS).all() and np.isposinf(z0[~full]).all()
    assert 0 < full.sum() < full.size


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_masks_and_values(hip, path):
    rng = np.random.default_rng(12)
    n = 1500
    pts = cloud(n, 13, 6.0, 4.0)
    values = R.wide_values(n, 14)
    values[::7] = np.nan
    values[1::41] = np.inf
    values[2::43] = -np.inf
    values[3::11] = 0.0
    values[4::13] = -0.0
    pts[::5, 2] = np.nan      # z is not consulted when values are given: these stay members
    pts[6::53, 0] = np.nan    # x or y that is not finite: never a member
    pts[8::59, 1] = -np.inf
    mask = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), n)
    stats = PATHS[path]
    kw = dict(origin=(0.0, 0.0), dim=(6, 4))
    got, r = check(hip, pts, 1.0, stats, values=values, mask=mask, what="values and mask", **kw)
    assert 0 < r.n_members < n
    check(hip, pts, 1.0, stats, values=values, what="values", **kw)
    check(hip, pts, 1.0, stats, mask=mask, what="mask", **kw)  # (z: its NaNs are no members now)
    check(hip, pts, 1.0, stats, mask=np.zeros(n, dtype=np.uint8), what="nothing masked in", **kw)
    # signed zeros alone in a cell: the minimum is -0.0 and the maximum +0.0, whichever comes first
    for z in ([0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]):
        got, _ = check(hip, np.array([[0.5, 0.5, v] for v in z]), 1.0, stats, what="zeros")
        assert (R.bits(got["min"])[0, 0], R.bits(got["max"])[0, 0]) == (0x8000000000000000, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "V", "packedH", "packedV", "external", "sliceH", "sliceV", "slicepackedV"])
def test_storages(hip, storage):
    pts = cloud(POINTS_PER_BLOCK + 37, 17)
    for stats in PATHS.values():
        check(hip, pts, 1.0, stats, storage=storage, what=storage)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_output_memory_and_determinism(hip, path):
    pts = cloud(2 * POINTS_PER_BLOCK + 3, 19)
    host, _ = check(hip, pts, 1.0, PATHS[path], what="host")
    dev, _ = check(hip, pts, 1.0, PATHS[path], device_out=True, what="device")
    again, _ = gpu_rasterize(hip, pts, 1.0, PATHS[path], device_out=True)
    for s in PATHS[path]:
        assert host[s].tobytes() == dev[s].tobytes() == again[s].tobytes(), s
    # a subset of the planes, in ascending bit order whatever the order of the names
    some = ("variance", "count") if path == "sorted" else ("max", "count")
    check(hip, pts, 1.0, some, device_out=True, what="subset")


@pytest.mark.gpu
def test_empty_and_all_nan_buffers(hip):
    """A caller's grid over an empty buffer is filled with the empty-cell values; a cloud without a finite point has no automatic grid."""
    import torch
    empty = _empty_buffer(hip)
    r = alg.rasterize(empty, 1.0, ALL, origin=(1.0, 2.0), dim=(5, 3))
    assert (r.origin, r.cols, r.rows, r.n_members) == ((1.0, 2.0), 5, 3, 0)
    assert not r.planes["count"].any() and R.bits(r.planes["count"]).max() == 0
    for s in ALL[1:]:
        assert (R.bits(r.planes[s]) == R.NAN_BITS).all() and r.planes[s].shape == (3, 5)
    pts = np.full((70, 3), np.nan)
    pts[:, 0] = 1.0
    d = torch.full((5, 4, 4), 123.0, dtype=torch.float64, device="cuda")
    r = alg.rasterize(make_buffer(hip, pts, "V"), 1.0, ALL, device_out_ptr=d.data_ptr())
    assert (r.origin, r.cols, r.rows, r.n_members) == ((0.0, 0.0), 0, 0, 0) and (d.cpu().numpy() == 123.0).all()  # untouched
    check(hip, pts, 1.0, ALL, origin=(0.0, 0.0), dim=(3, 3), values=np.ones(70), what="no finite y")


# ---- the fill

def gpu_fill(a, h, hip=None):
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    rows, cols = a.shape
    d_in = torch.from_numpy(a).cuda()
    d_out = torch.full((rows, cols), 123.0, dtype=torch.float64, device="cuda")
    alg.grid_fill(d_in.data_ptr(), d_out.data_ptr(), cols, rows, h, hip)
    out = d_out.cpu().numpy()
    assert np.array_equal(R.bits(d_in.cpu().numpy()), R.bits(a))  # the input is not written
    return out


def holed(cols, rows, empty_fraction, seed):
    rng = np.random.default_rng(seed)
    a = R.wide_values(cols * rows, seed).reshape(rows, cols)
    a[rng.random((rows, cols)) < empty_fraction] = R.NAN
    if empty_fraction >= 1.0:
        a[:] = R.NAN
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("h", [0, 1, 15, 16])
@pytest.mark.parametrize("empty_fraction", [0.0, 0.5, 0.95, 1.0])
def test_fill(hip, h, empty_fraction):
    a = holed(TILE_COLS + 7, TILE_ROWS + 5, empty_fraction, 50 + h)
    if 0.0 < empty_fraction < 1.0:
        a[3, 4], a[20, TILE_COLS] = np.inf, -np.inf  # empty like a NaN
        a[10, 10] = -0.0
        a[10, 11] = R.NAN
    got, want = gpu_fill(a, h, hip), R.fill(a, h)
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert bad.size == 0, f"{len(bad)} cells differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"
    finite = np.isfinite(a)
    assert np.array_equal(R.bits(got[finite]), R.bits(a[finite]))  # finite entries keep their bits
    if empty_fraction == 1.0:
        assert (R.bits(got) == R.NAN_BITS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(1, 1), (3, 1), (1, 5), (7, 40), (150, 3), (TILE_COLS, TILE_ROWS), (TILE_COLS + 1, TILE_ROWS + 1), (2 * TILE_COLS + 1, 2 * TILE_ROWS + 1)])
def test_fill_raster_sizes(hip, cols, rows):
    """rasters narrower than the half-width, and around the tile"""
    a = holed(cols, rows, 0.6, cols + rows)
    for h in (2, MAX_FILL):
        assert np.array_equal(R.bits(gpu_fill(a, h, hip)), R.bits(R.fill(a, h))), h


@pytest.mark.gpu
def test_fill_refusals_on_the_device(hip):
    import torch
    d = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    assert _code(lambda: alg.grid_fill(d.data_ptr(), d.data_ptr(), 4, 4, 1, hip)) == 1  # in place
    assert _code(lambda: alg.grid_fill(d.data_ptr(), d.data_ptr() + 8, 4, 3, MAX_FILL + 1, hip)) == 1


# ---- the Python layer, the example

@pytest.mark.gpu
def test_python_layer(hip):
    import torch
    rng = np.random.default_rng(23)
    n = 2000
    pts = cloud(n, 24, 9.0, 6.0)
    intensity = rng.integers(0, 65536, n).astype(np.uint16)
    buf = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY], api=hip))
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
    buf.set_attribute_range(A.INTENSITY, range(0, n), intensity)
    names = ("mean", "stdev", "variance", "count", "max")
    r = alg.rasterize(buf, 1.0, names, values=A.INTENSITY)
    want, members, grid = R.rasterize(pts, 1.0, ALL, values=intensity.astype(np.float64))
    assert list(r.planes) == list(names) and r.n_members == members == n and (r.origin[0], r.origin[1], r.cols, r.rows) == grid
    assert_planes(r.planes, want, ("mean", "variance", "count", "max"), "intensity")
    with np.errstate(invalid="ignore"):
        assert np.array_equal(R.bits(r.planes["stdev"]), R.bits(np.sqrt(want["variance"])))
    assert np.array_equal(R.bits(alg.rasterize(buf, 1.0, "stdev", values=A.INTENSITY).planes["stdev"]), R.bits(r.planes["stdev"]))
    # the planes in device memory, then the fill on them
    d = torch.full((2, r.rows, r.cols), 123.0, dtype=torch.float64, device="cuda")
    rd = alg.rasterize(buf, 1.0, ("max", "min"), device_out_ptr=d.data_ptr())
    assert rd.planes == {} and (rd.cols, rd.rows, rd.n_members) == (r.cols, r.rows, n)
    z = R.rasterize(pts, 1.0, ("min", "max"))[0]
    assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(np.stack([z["min"], z["max"]])))
    filled = torch.empty((r.rows, r.cols), dtype=torch.float64, device="cuda")
    alg.grid_fill(d[1].data_ptr(), filled.data_ptr(), r.cols, r.rows, 3)
    assert np.array_equal(R.bits(filled.cpu().numpy()), R.bits(R.fill(z["max"], 3)))


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/canopy_height_model.py: the tallest canopy cell over every planted object is the height it was built with, within the bound
    tests/test_hag.py derives for examples/height_above_ground.py (the ground under a roof point is a convex combination of ground points
    within the box's half-sizes plus 1.5 m of its centre; slopes 0.12 and 1.5 / 18, noise 0.1)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("canopy_height_model", os.path.join(root, "examples", "canopy_height_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(60000)
    assert result["n_unresolved"] == 0 and result["surface_members"] == result["n_points"]
    assert [f["object"] for f in result["found"]] == list(range(len(mod.scene_module.OBJECTS)))
    for f in result["found"]:
        _, _, sx, sy, h = mod.scene_module.OBJECTS[f["object"]]
        assert f["built"] == mod.scene_module.CLEAR + h
        bound = 0.12 * (sx / 2 + 1.5) + (1.5 / 18.0) * (sy / 2 + 1.5) + 0.1
        assert abs(f["tallest"] - f["built"]) <= bound, (f, bound)
