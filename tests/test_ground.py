"""Ground classification by the progressive morphological filter (pst_pmf_schedule, pst_pmf_grid, pst_pmf_ground_mask,
pst_grid_morphology_device, pst_finite_mask_device, pst_buffer_set_u8_where_device, pst_pmf_kernel_shape) against tests/pmf_ref.py.

CPU tests pin the schedule, the restatement on a hand-computed raster and on the recorded scene, and the argument checks answered on the host.
GPU tests compare the HIP path with the restatement: the mask, the count and the three rasters with np.array_equal, no tolerance anywhere --
the result is made of minima, maxima and one f64 addition per cell and window, which numpy evaluates with the same roundings."""
import ctypes as C
import os

import numpy as np
import pytest

import pmf_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

POINTS_PER_BLOCK = 1024  # asserted against pst_pmf_kernel_shape below: the parametrisations need them at collection time
TILE_COLS = 64
TILE_ROWS = 32
MAX_HALF_WIDTH = 32
SEAM_COUNTS = [1, 2, POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 5]
SCENE_PARAMS = alg.PmfParameters(1.0, 17.0, 1.0, 0.5, 3.0)


def ref_schedule(p):
    return R.schedule(p.cell_size, p.max_window_size, p.slope, p.initial_distance, p.max_distance, p.exponential, p.base)


def ref_ground(pts, p):
    hs, ths = ref_schedule(p)
    return R.ground(pts, hs, ths, p.cell_size)


def terrain(n, seed, cols=24.0, rows=17.0):
    """n points over cols x rows: a rolling surface, a lifted block and a few high strays (more than one window separates them)."""
    rng = np.random.default_rng(seed)
    x, y = rng.random(n) * cols, rng.random(n) * rows
    z = 0.04 * x + 0.8 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.normal(0.0, 0.02, n)
    block = (x > 0.3 * cols) & (x < 0.55 * cols) & (y > 0.25 * rows) & (y < 0.6 * rows)
    z = np.where(block, z + 3.5, z)
    z = np.where(rng.random(n) < 0.03, z + rng.uniform(0.3, 5.0, n), z)
    return np.column_stack([x, y, z])


def raster_cloud(cols, rows, seed, per_cell=2.0, cell=1.0):
    """A cloud whose raster has exactly cols x rows cells of edge `cell`: two corner points pin the extent, and about a tenth of the cells stay empty."""
    n = max(int(cols * rows * per_cell), 1)
    pts = terrain(n, seed, cols * cell, rows * cell)
    pts[:, 0] = np.minimum(pts[:, 0], (cols - 0.5) * cell)
    pts[:, 1] = np.minimum(pts[:, 1], (rows - 0.5) * cell)
    pts = np.concatenate([pts, [[0.0, 0.0, 0.1], [(cols - 0.5) * cell, (rows - 0.5) * cell, 0.2]]])
    _, _, _, got_rows, got_cols, _ = R.cells_of(pts, cell)
    assert (got_cols, got_rows) == (cols, rows)
    return pts


def gpu_ground(hip, pts, p, storage="H", device=False):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip, kind=HashMapBuffer if storage.endswith("H") else VectorBuffer)
    if not device:
        mask, count, surf = alg.ground_mask(buf, p, return_surfaces=True)
        assert mask.dtype == np.uint8 and mask.shape == (buf.len(),)
        return mask, count, surf
    import torch
    d = torch.full((max(buf.len(), 1),), 7, dtype=torch.uint8, device="cuda")
    none, count, surf = alg.ground_mask(buf, p, device_mask_ptr=d.data_ptr(), return_surfaces=True)
    assert none is None
    return d.cpu().numpy()[:buf.len()], count, surf


def assert_same(got, want, what=""):
    (gm, gc, gs), (wm, wc, ws) = got, want
    for name in ("min_z", "opened", "limit"):
        assert gs[name].shape == ws[name].shape, f"{what}: {name} is {gs[name].shape}, not {ws[name].shape}"
        bad = np.argwhere(gs[name] != ws[name])
        assert bad.size == 0, f"{what}: {len(bad)} cells of {name} differ, first at {bad[:3].tolist()}: {gs[name][tuple(bad[0])]} vs {ws[name][tuple(bad[0])]}"
    bad = np.flatnonzero(gm != wm)
    assert bad.size == 0, f"{what}: {bad.size} of {len(wm)} mask bytes differ, first at {bad[:4]}"
    assert gc == wc, f"{what}: count {gc} vs {wc}"


def check(hip, pts, p, storage="H", device=False, what=""):
    want = ref_ground(pts, p)
    assert_same(gpu_ground(hip, pts, p, storage, device), want, what)
    return want


# ------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_schedule(hip):
    def same(p):
        (h, th), (rh, rth) = alg.pmf_schedule(p, hip), ref_schedule(p)
        assert h.dtype == np.uint32 and th.dtype == np.float64
        assert np.array_equal(h, rh) and np.array_equal(th, rth), (p, h, th, rh, rth)
        return h.tolist(), th.tolist()
    assert same(SCENE_PARAMS) == ([1, 2, 4, 8], [0.5, 2.5, 3.0, 3.0])
    assert same(alg.PmfParameters(1.0, 33.0, 1.0, 0.5, 3.0))[0] == [1, 2, 4, 8, 16]
    assert len(same(alg.PmfParameters())[0]) == 5
    # linear: h = 2, 4, 6, 8; every step widens the window by 4 cells
    assert same(alg.PmfParameters(1.0, 17.0, 0.3, 0.5, 3.0, False, 2)) == ([2, 4, 6, 8], [0.5, 0.3 * 4.0 * 1.0 + 0.5, 0.3 * 4.0 * 1.0 + 0.5, 0.3 * 4.0 * 1.0 + 0.5])
    assert same(alg.PmfParameters(0.1, 2.0, 1.0, 0.15, 2.5, False, 3))[0] == [3, 6, 9, 12]
    assert same(alg.PmfParameters(0.5, 0.0, 1.0, 0.15, 2.5))[0] == [1]  # the first window always runs
    assert same(alg.PmfParameters(2.5, 70.0, 0.7, 0.1, 1.9, True, 3))[0] == [1, 3, 9, 27]
    # the cap: 32 linear windows of base 1 reach w = 65; one more is refused
    assert same(alg.PmfParameters(1.0, 65.0, 1.0, 0.1, 1.0, False, 1))[0] == list(range(1, 33))
    for p in (alg.PmfParameters(1.0, 65.5, 1.0, 0.1, 1.0, False, 1), alg.PmfParameters(1.0, 1e12, 1.0, 0.1, 1.0)):
        assert _code(lambda: alg.pmf_schedule(p, hip)) == 1
        with pytest.raises(ValueError):
            ref_schedule(p)


def test_restatement_on_a_hand_computed_raster(hip):
    """Flat ground at z = 0, one point per cell of 12 x 12, with a block of 3 x 3 cells at z = 5.  h = 1 (a 3 x 3 window) leaves the block
    standing; h = 2 opens it away.  So with the windows h = 1, 2 the block's points are ground iff 5 <= th_1."""
    g = np.arange(12) + 0.5
    pts = np.array([[x, y, 5.0 if 4 <= x < 7 and 5 <= y < 8 else 0.0] for y in g for x in g])
    block = pts[:, 2] == 5.0
    z0 = R.min_raster(pts, 1.0)
    assert z0.shape == (12, 12) and (z0 == 5.0).sum() == 9 and np.array_equal(z0[5:8, 4:7], np.full((3, 3), 5.0))
    for h in (0, 1, 2, 3, 11, 40):
        assert np.array_equal(R.erode(z0, h), R.erode_brute(z0, h)) and np.array_equal(R.dilate(z0, h), R.dilate_brute(z0, h)), h
    assert np.array_equal(R.erode(z0, 1)[6, 5], 5.0) and (R.erode(z0, 1) == 5.0).sum() == 1     # only the block's centre survives the erosion
    assert np.array_equal(R.dilate(R.erode(z0, 1), 1), z0)                                      # ... and the dilation puts the block back
    assert not R.dilate(R.erode(z0, 2), 2).any()                                                # a 5 x 5 window opens it away
    holes = z0.copy()
    holes[0, :] = np.inf
    holes[3, 3] = np.inf
    assert np.array_equal(R.dilate(holes, 1)[0, :], np.zeros(12)) and R.dilate(holes, 1)[3, 3] == 0.0  # empty cells are ignored, and filled
    assert np.isinf(R.dilate(np.full((3, 4), np.inf), 2)).all() and np.isinf(R.erode(holes, 0)[0]).all()
    for dmax, block_is_ground in ((3.0, False), (4.999, False), (5.0, True), (7.0, True)):
        p = alg.PmfParameters(1.0, 5.0, 10.0, 0.5, dmax)
        hs, ths = alg.pmf_schedule(p, hip)
        assert hs.tolist() == [1, 2] and ths.tolist() == [0.5, dmax]
        mask, count, surf = R.ground(pts, hs, ths, 1.0)
        assert mask[~block].all() and mask[block].all() == block_is_ground and mask[block].any() == block_is_ground
        assert count == 144 - (0 if block_is_ground else 9) and not surf["opened"].any()
        assert np.array_equal(surf["limit"], np.minimum(z0 + 0.5, dmax))


def test_restatement_on_the_recorded_scene(hip):
    pts, roof, pole = R.scene()
    hs, ths = alg.pmf_schedule(SCENE_PARAMS, hip)
    mask, count, _ = R.ground(pts, hs, ths, 1.0)
    ground = ~roof & ~pole
    assert roof.sum() > 500 and pole.sum() >= 3
    assert not mask[roof].any() and not mask[pole].any()
    assert mask[ground].mean() >= 0.99
    assert count == int(mask[ground].sum())


# ----------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype), A.CLASSIFICATION], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _params(*a):
    return alg.PmfParameters(*a).c_args()


def test_kernel_shape(hip):
    assert alg.pmf_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK, "tile_cols": TILE_COLS, "tile_rows": TILE_ROWS, "max_half_width": MAX_HALF_WIDTH}
    one = C.c_uint32(7)
    hip.pmf_kernel_shape(None, None, None, C.byref(one))  # each pointer is optional
    assert one.value == MAX_HALF_WIDTH
    hip.pmf_kernel_shape(None, None, None, None)
    assert alg.pmf_phase_times(hip) == (0.0, 0.0, 0.0)


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments, invalid parameters, a missing position and an empty buffer: the same answer with or without a device, because no device
    is looked for."""
    buf = _empty_buffer(hip)
    mask, count = (C.c_uint8 * 8)(), C.c_uint64(9)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    n, good = C.byref(count), _params()
    nan, inf = float("nan"), float("inf")

    def call(params, b=buf._h, m=mask, mk=1, sk=1, out=n):
        return lambda: hip.pmf_ground_mask(b, *params, m, mk, None, sk, out)
    assert _code(call(good, b=None)) == 1 and _code(call(good, m=None)) == 1 and _code(call(good, out=None)) == 1
    assert _code(call(good, mk=7)) == 1 and _code(call(good, sk=2)) == 1  # no such memory kind
    for cell in (0.0, -1.0, nan, inf, -inf):
        assert _code(call(_params(cell))) == 1, cell
        assert _code(lambda: hip.pmf_grid(buf._h, cell, (C.c_double * 2)(), (C.c_uint32 * 2)(), n)) == 1
    for bad in (-1.0, -1e-300, nan, inf, -inf):
        for at in range(1, 5):  # max_window_size, slope, initial_distance, max_distance
            values = [1.0, 33.0, 1.0, 0.15, 2.5]
            values[at] = bad
            assert _code(call(_params(*values))) == 1, values
    for exponential, base in ((True, 0), (True, 1), (False, 0)):
        assert _code(call(_params(1.0, 33.0, 1.0, 0.15, 2.5, exponential, base))) == 1
    assert _code(call(_params(1.0, 1e9, 1.0, 0.15, 2.5, False, 1))) == 1  # more than 32 windows
    # a position that is not Vec3f64 is known from the layout alone
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(call(good, b=f32._h)) == 4
    assert _code(lambda: hip.pmf_grid(f32._h, 1.0, (C.c_double * 2)(), (C.c_uint32 * 2)(), n)) == 4
    assert _code(lambda: hip.finite_mask_device(f32._h, fake)) == 4
    with pytest.raises(PasturePanic):
        call(good, b=f32._h)()
    # an empty buffer is answered on the host: no ground, nothing written
    for kind in (HashMapBuffer, VectorBuffer):
        empty = _empty_buffer(hip, kind=kind)
        count.value = 9
        call(good, b=empty._h)()
        assert count.value == 0
        assert alg.ground_mask(empty)[1] == 0 and alg.ground_mask(empty)[0].shape == (0,)
        assert alg.pmf_grid(empty, 1.0) == {"origin": (0.0, 0.0), "cols": 0, "rows": 0, "n_finite": 0}
        assert alg.classify_ground(empty) == 0
        hip.finite_mask_device(empty._h, None)
        hip.buffer_set_u8_where_device(empty._h, b"Classification", None, 2)
        assert _code(lambda: hip.buffer_set_u8_where_device(empty._h, b"Intensity", fake, 2)) == 4        # no such attribute
        assert _code(lambda: hip.buffer_set_u8_where_device(empty._h, b"Position3D", fake, 2)) == 4       # not a U8 attribute
        assert _code(lambda: hip.buffer_set_u8_where_device(empty._h, None, fake, 2)) == 1
    assert _code(lambda: hip.buffer_set_u8_where_device(None, b"Classification", fake, 2)) == 1
    # the morphology: an operation that does not exist, null rasters, in place; a raster without cells is answered on the host
    assert _code(lambda: hip.grid_morphology_device(fake, C.c_void_p(16), 4, 4, 1, 2)) == 1
    assert _code(lambda: hip.grid_morphology_device(None, fake, 4, 4, 1, 0)) == 1
    assert _code(lambda: hip.grid_morphology_device(fake, None, 4, 4, 1, 0)) == 1
    assert _code(lambda: hip.grid_morphology_device(fake, fake, 4, 4, 1, 0)) == 1
    assert _code(lambda: hip.grid_morphology_device(fake, C.c_void_p(16), 1 << 15, (1 << 13) + 1, 1, 0)) == 23
    hip.grid_morphology_device(None, None, 0, 4, 1, 0)
    hip.grid_morphology_device(None, None, 4, 0, 1, 1)
    assert _code(lambda: hip.pmf_schedule(*good, None, None, None)) == 1
    windows = C.c_uint32()
    hip.pmf_schedule(*good, None, None, C.byref(windows))  # each array is optional
    assert windows.value == 5
    assert _code(lambda: hip.pmf_phase_times(None)) == 1


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PastureError) as e:
        hip.grid_morphology_device(C.c_void_p(8), C.c_void_p(4096), 4, 4, 1, 0)
    assert e.value.code == 21 and "no CPU fallback" in str(e.value)


# -------------------------------------------------------------------------------------------------------------------------------- GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_point_counts_around_the_seams(hip, n):
    """Both storages, interleaved records with the position at byte 1 and at byte 2, a slice; the mask in host and in device memory."""
    pts = terrain(n, 20 + n % 7, 40.0, 30.0)
    p = alg.PmfParameters(1.0, 9.0, 1.0, 0.3, 2.0)
    want = ref_ground(pts, p)
    if n >= POINTS_PER_BLOCK - 1:
        assert 0 < want[1] < n and np.isinf(want[2]["min_z"]).any(), "the case is to have ground, other points and empty cells"
    for storage, device in (("H", False), ("V", True), ("external", False), ("packedV", True), ("packedH", False), ("sliceV", False), ("sliceH", True)):
        assert_same(gpu_ground(hip, pts, p, storage, device), want, f"{n} {storage} {'device' if device else 'host'}")


@pytest.mark.gpu
def test_empty_and_non_finite_clouds(hip):
    for device in (False, True):
        mask, count, surf = gpu_ground(hip, np.zeros((0, 3)), SCENE_PARAMS, device=device)
        assert mask.shape == (0,) and count == 0 and surf["limit"].shape == (0, 0)
        mask, count, surf = gpu_ground(hip, np.full((POINTS_PER_BLOCK + 3, 3), np.nan), SCENE_PARAMS, "V", device=device)
        assert not mask.any() and mask.shape == (POINTS_PER_BLOCK + 3,) and count == 0 and surf["min_z"].shape == (0, 0)


def _axis_sizes(tile):
    return [1, 2, tile - 1, tile, tile + 1, 2 * tile + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(1, 1), (1, 150), (150, 1)] + [(c, 5) for c in _axis_sizes(TILE_COLS)[1:]] + [(7, r) for r in _axis_sizes(TILE_ROWS)[1:]]
                         + [(2 * TILE_COLS + 3, 2 * TILE_ROWS + 3), (TILE_COLS, TILE_ROWS), (TILE_COLS + 1, TILE_ROWS + 1)])
def test_raster_sizes_around_the_tile(hip, cols, rows):
    pts = raster_cloud(cols, rows, cols * 1000 + rows)
    p = alg.PmfParameters(1.0, 17.0, 0.5, 0.25, 2.0)
    want = check(hip, pts, p, "H" if (cols + rows) % 2 else "V", what=f"{cols} x {rows}")
    assert want[2]["min_z"].shape == (rows, cols)
    buf = make_buffer(hip, pts, "H")
    grid = alg.pmf_grid(buf, 1.0)
    assert grid == {"origin": (0.0, 0.0), "cols": cols, "rows": rows, "n_finite": len(pts)}


def _random_raster(rows, cols, empty, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 10.0, (rows, cols))
    a[rng.random((rows, cols)) < empty] = np.inf
    return a


def gpu_morphology(hip, a, h, dilate):
    import torch
    rows, cols = a.shape
    d_in = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_out = torch.full((rows, cols), float("nan"), dtype=torch.float64, device="cuda")
    (alg.grid_dilate if dilate else alg.grid_erode)(d_in.data_ptr(), d_out.data_ptr(), cols, rows, h, api=hip)
    assert np.array_equal(d_in.cpu().numpy(), a), "the input is not written"
    return d_out.cpu().numpy()


def check_morphology(hip, a, h, what=""):
    for dilate, ref in ((False, R.erode), (True, R.dilate)):
        got, want = gpu_morphology(hip, a, h, dilate), ref(a, h)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what} {'dilate' if dilate else 'erode'} h = {h}: {len(bad)} cells differ, first at {bad[:3].tolist()}"


_H = MAX_HALF_WIDTH


@pytest.mark.gpu
@pytest.mark.parametrize("empty", [0.0, 0.5, 0.95])
@pytest.mark.parametrize("h", [0, 1, 2, _H - 1, _H, _H + 1, 2 * _H + 3])
def test_half_widths_around_the_pass_limit(hip, h, empty):
    """2 tiles and a ragged third on each axis; half-widths that need one, two and three passes per axis"""
    a = _random_raster(2 * TILE_ROWS + 9, 2 * TILE_COLS + 11, empty, 31 + h)
    check_morphology(hip, a, h, f"{int(empty * 100)} % empty")


@pytest.mark.gpu
def test_half_widths_at_and_beyond_the_raster(hip):
    for rows, cols in ((13, 20), (1, 1), (1, 97), (97, 1), (TILE_ROWS + 1, 3)):
        a = _random_raster(rows, cols, 0.5, rows * 100 + cols)
        for h in sorted({1, rows - 1, rows, rows + 1, cols - 1, cols, cols + 1, 2 * _H + 3, 1000, 2 ** 32 - 1} - {-1, 0}):
            check_morphology(hip, a, h, f"{rows} x {cols}")


@pytest.mark.gpu
def test_empty_rows_columns_and_rasters(hip):
    a = _random_raster(2 * TILE_ROWS + 3, TILE_COLS + 5, 0.2, 77)
    a[10:10 + 2 * 3 + 2, :] = np.inf   # a band of 8 empty rows: h = 3 does not bridge it, h = 4 does
    a[:, 30:41] = np.inf               # 11 empty columns
    a[:, 0] = np.inf
    a[-1, :] = np.inf
    for h in (1, 3, 4, 5, 6, _H + 1):
        check_morphology(hip, a, h, "bands")
    nothing = np.full((TILE_ROWS + 2, TILE_COLS + 2), np.inf)
    for h in (1, _H + 1):
        assert np.isinf(gpu_morphology(hip, nothing, h, False)).all() and np.isinf(gpu_morphology(hip, nothing, h, True)).all()
    one = nothing.copy()
    one[5, 7] = -3.0
    check_morphology(hip, one, 2, "a single cell")
    assert (gpu_morphology(hip, one, 2, True) == -3.0).sum() == 25 and (gpu_morphology(hip, one, 2, False) == -3.0).sum() == 25


@pytest.mark.gpu
def test_large_windows_in_the_filter(hip):
    """Windows beyond the pass limit and beyond the raster inside pst_pmf_ground_mask: h = 3, 9, 27, 81 on 70 x 40 cells."""
    pts = raster_cloud(70, 40, 5)
    p = alg.PmfParameters(1.0, 150.0, 0.2, 0.2, 2.5, True, 3)
    assert alg.pmf_schedule(p, hip)[0].tolist() == [1, 3, 9, 27, 81]
    check(hip, pts, p, what="exponential base 3")
    p = alg.PmfParameters(0.5, 40.0, 0.1, 0.2, 2.5, False, 11)
    assert alg.pmf_schedule(p, hip)[0].tolist() == [11, 22, 33, 44]
    check(hip, pts, p, "V", what="linear base 11, cell 0.5")


@pytest.mark.gpu
def test_threshold_knife_edge(hip):
    """A point whose z equals the limit of its cell, by the same f64 expression, is ground; the next double above it is not."""
    base = terrain(3000, 41)
    p = alg.PmfParameters(1.0, 9.0, 0.7, 0.3, 1.1)
    _, _, surf = ref_ground(base, p)
    _, row, col, _, _, _ = R.cells_of(base, 1.0)
    limit, z0 = surf["limit"], surf["min_z"]
    # cells whose limit is not below their lowest point: a point AT the limit changes neither the raster nor the limit
    at = [i for i in range(0, 3000, 37) if limit[row[i], col[i]] >= z0[row[i], col[i]]][:40]
    assert len(at) >= 20
    on = np.array([[base[i, 0], base[i, 1], limit[row[i], col[i]]] for i in at])
    above = on.copy()
    above[:, 2] = np.nextafter(on[:, 2], np.inf)
    pts = np.concatenate([base, on, above])
    want = ref_ground(pts, p)
    assert np.array_equal(want[2]["limit"], limit)
    assert want[0][3000:3000 + len(at)].all() and not want[0][3000 + len(at):].any()
    for storage in ("H", "packedV"):
        assert_same(gpu_ground(hip, pts, p, storage), want, "at and above the limit")


@pytest.mark.gpu
def test_cell_knife_edge(hip):
    """Points on a lattice of step 0.1 with cell_size 0.1: (x - x0) / cell_size is an exact integer for some and one ulp below for others."""
    j = np.arange(60, dtype=np.float64)
    for x0 in (0.0, 0.3, -7.1):
        coord = x0 + j * 0.1
        q = (coord - coord.min()) / 0.1
        assert (q == np.round(q)).sum() > 10 and (q < np.round(q)).sum() > 0, "both kinds of quotient are in the case"
        x, y = np.meshgrid(coord, coord[:41])
        rng = np.random.default_rng(3)
        z = 0.3 * np.sin(x) + np.where(rng.random(x.shape) < 0.1, 2.0, 0.0)
        pts = np.column_stack([x.ravel(), y.ravel(), z.ravel()])[rng.permutation(x.size)]
        check(hip, pts, alg.PmfParameters(0.1, 1.7, 1.0, 0.05, 0.5), what=f"lattice at {x0}")


@pytest.mark.gpu
def test_duplicates_and_equal_minima(hip):
    pts = terrain(2000, 43)
    pts = np.concatenate([pts, pts[:700], pts[:700]])  # every one of 700 points three times
    pts[1000:1400, 2] = np.round(pts[1000:1400, 2], 1)  # many equal z, some of them the minimum of their cell
    pts = pts[np.random.default_rng(44).permutation(len(pts))]
    check(hip, pts, alg.PmfParameters(1.0, 9.0, 1.0, 0.3, 2.0), what="duplicates")
    same = np.tile([[3.25, 4.5, 1.75]], (POINTS_PER_BLOCK + 9, 1))  # one place, one cell
    mask, count, surf = gpu_ground(hip, same, SCENE_PARAMS, "V")
    assert mask.all() and count == len(same) and surf["min_z"].tolist() == [[1.75]] and surf["limit"].tolist() == [[2.25]]


@pytest.mark.gpu
def test_signed_zeros(hip):
    """Flat ground at z = +-0.0 and a threshold of 0: the rasters compare as values, and z = +0.0 is not above a limit of -0.0."""
    rng = np.random.default_rng(45)
    n = 3000
    pts = np.column_stack([rng.random(n) * 20, rng.random(n) * 20, np.where(rng.random(n) < 0.5, 0.0, -0.0)])
    pts[::50, 2] = 1.0
    p = alg.PmfParameters(1.0, 9.0, 0.0, 0.0, 0.0)
    want = check(hip, pts, p, what="+-0.0")
    assert np.array_equal(want[0], pts[:, 2] != 1.0) and not want[2]["limit"].any()


@pytest.mark.gpu
def test_non_finite_points(hip):
    pts = terrain(4000, 46)
    rng = np.random.default_rng(47)
    bad = rng.choice(4000, 180, replace=False)
    k = 0
    for coord in range(3):
        for value in (np.nan, np.inf, -np.inf):
            pts[bad[k:k + 20], coord] = value
            k += 20
    good = np.isfinite(pts).all(axis=1)
    assert (~good).sum() == 180
    p = alg.PmfParameters(1.0, 9.0, 1.0, 0.3, 2.0)
    sub = ref_ground(pts[good], p)  # the finite subset, mapped back
    want_mask = np.zeros(4000, dtype=np.uint8)
    want_mask[good] = sub[0]
    for storage, device in (("H", False), ("external", True)):
        assert_same(gpu_ground(hip, pts, p, storage, device), (want_mask, sub[1], sub[2]), "non-finite")
    assert_same((want_mask, sub[1], sub[2]), ref_ground(pts, p), "the restatement on the whole cloud")
    buf = make_buffer(hip, pts, "V")
    assert alg.pmf_grid(buf, 1.0)["n_finite"] == 4000 - 180


@pytest.mark.gpu
def test_dense_cell_in_descending_order(hip):
    """10^5 points in one cell, every one lower than all before it: no filtered atomic can be skipped on a fresh read."""
    n = 100_000
    rng = np.random.default_rng(48)
    pts = np.column_stack([rng.random(n) * 0.9, rng.random(n) * 0.9, np.linspace(100.0, 0.0, n)])
    mask, count, surf = gpu_ground(hip, pts, SCENE_PARAMS)
    assert surf["min_z"].tolist() == [[0.0]] and surf["opened"].tolist() == [[0.0]] and surf["limit"].tolist() == [[0.5]]
    assert np.array_equal(mask, pts[:, 2] <= 0.5) and count == int((pts[:, 2] <= 0.5).sum()) and 0 < count < n


_SCENE = {}


def scene_case():
    if not _SCENE:
        pts, roof, pole = R.scene()
        want = ref_ground(pts, SCENE_PARAMS)
        for a in (pts, roof, pole, want[0], *want[2].values()):
            a.setflags(write=False)
        _SCENE["case"] = (pts, roof, pole, want)
    return _SCENE["case"]


@pytest.mark.gpu
def test_recorded_scene_and_determinism(hip):
    pts, roof, pole, want = scene_case()
    buf = make_buffer(hip, pts, "H")
    first = alg.ground_mask(buf, SCENE_PARAMS, return_surfaces=True)
    second = alg.ground_mask(buf, SCENE_PARAMS, return_surfaces=True)
    assert_same(first, want, "the recorded scene")
    assert not first[0][roof].any() and not first[0][pole].any() and first[0][~roof & ~pole].mean() >= 0.99
    assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]
    for name in ("min_z", "opened", "limit"):
        assert first[2][name].tobytes() == second[2][name].tobytes(), name
    assert first[2]["origin"] == (pts[:, 0].min(), pts[:, 1].min()) and first[2]["cell_size"] == 1.0
    assert alg.ground_mask(buf, SCENE_PARAMS)[1] == want[1]  # without the surfaces


def _classified_buffer(hip, pts, kind, classes):
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY, A.CLASSIFICATION], api=hip)
    buf = kind.new_from_layout(layout)
    n = len(pts)
    buf.resize(n)
    buf.set_attribute_range(A.POSITION_3D, range(0, n), np.ascontiguousarray(pts))
    buf.set_attribute_range(A.INTENSITY, range(0, n), (np.arange(n) * 7 % 65521).astype(np.uint16))
    buf.set_attribute_range(A.CLASSIFICATION, range(0, n), classes)
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [HashMapBuffer, VectorBuffer])
def test_classify_ground(hip, kind):
    pts, _, _, want = scene_case()
    pts = pts[:20000].copy()
    pts[5::1000, 1] = np.nan
    want = ref_ground(pts, SCENE_PARAMS)
    ground = want[0] == 1
    classes = (np.arange(len(pts)) % 7 + 10).astype(np.uint8)
    buf = _classified_buffer(hip, pts, kind, classes)
    assert alg.classify_ground(buf, SCENE_PARAMS) == want[1]
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), np.where(ground, 2, classes))   # the other points keep their class
    assert np.array_equal(buf.view_attribute(A.INTENSITY), (np.arange(len(pts)) * 7 % 65521).astype(np.uint16))
    assert np.array_equal(buf.view_attribute(A.POSITION_3D)[ground], pts[ground])
    assert alg.classify_ground(buf, SCENE_PARAMS, ground_class=9, other_class=1) == want[1]
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), np.where(ground, 9, 1))
    no_class = make_buffer(hip, pts, "H")
    assert _code(lambda: alg.classify_ground(no_class, SCENE_PARAMS)) == 4


@pytest.mark.gpu
def test_remove_and_extract_ground_partition_the_finite_points(hip):
    pts, _, _, _ = scene_case()
    pts = pts[:20000].copy()
    pts[7::500, 0] = np.inf
    pts[9::500, 2] = np.nan
    want = ref_ground(pts, SCENE_PARAMS)
    ground, finite = want[0] == 1, np.isfinite(pts).all(axis=1)
    intensity = (np.arange(len(pts)) * 7 % 65521).astype(np.uint16)
    buf = _classified_buffer(hip, pts, HashMapBuffer, np.zeros(len(pts), dtype=np.uint8))
    kept, n_ground = alg.extract_ground(buf, SCENE_PARAMS)
    rest, n_ground2 = alg.remove_ground(buf, SCENE_PARAMS)
    assert n_ground == n_ground2 == want[1] == kept.len() and kept.len() + rest.len() == int(finite.sum()) < len(pts)
    assert np.array_equal(kept.view_attribute(A.POSITION_3D), pts[ground]) and np.array_equal(kept.view_attribute(A.INTENSITY), intensity[ground])
    assert np.array_equal(rest.view_attribute(A.POSITION_3D), pts[finite & ~ground]) and np.array_equal(rest.view_attribute(A.INTENSITY), intensity[finite & ~ground])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_set_u8_where_and_finite_mask_around_the_seams(hip, n):
    import torch
    rng = np.random.default_rng(n)
    pts = terrain(n, 49)
    pts[rng.random(n) < 0.2, rng.integers(0, 3)] = np.nan
    classes = rng.integers(0, 256, n).astype(np.uint8)
    mask = rng.choice(np.array([0, 0, 1, 255], dtype=np.uint8), n)
    d_mask = torch.from_numpy(mask).cuda()
    for kind in (HashMapBuffer, VectorBuffer):
        buf = _classified_buffer(hip, pts, kind, classes)
        alg.set_u8_where(buf, A.CLASSIFICATION, d_mask.data_ptr(), 77)
        assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), np.where(mask != 0, 77, classes))
        assert np.array_equal(buf.view_attribute(A.INTENSITY), (np.arange(n) * 7 % 65521).astype(np.uint16)), "the neighbouring bytes of the record"
        d_finite = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        alg.finite_mask(buf, d_finite.data_ptr())
        assert np.array_equal(d_finite.cpu().numpy(), np.isfinite(pts).all(axis=1).astype(np.uint8))


@pytest.mark.gpu
def test_a_raster_that_is_too_large_is_refused(hip):
    far = np.array([[0.0, 0.0, 0.0], [20000.0, 20000.0, 1.0]])  # 4 x 10^8 cells of edge 1
    buf = make_buffer(hip, far, "H")
    for p in (alg.PmfParameters(), alg.PmfParameters(1e-3)):
        with pytest.raises(PastureError) as e:
            alg.ground_mask(buf, p)
        assert e.value.code == 23 and "larger cell" in str(e.value)
    assert _code(lambda: alg.pmf_grid(buf, 1.0)) == 23
    assert _code(lambda: alg.pmf_grid(make_buffer(hip, np.array([[-1.5e308, 0.0, 0.0], [1.5e308, 1.0, 1.0]]), "H"), 1.0)) == 23  # the extent overflows
    # 2^14 x 2^14 cells are exactly 2^28: the geometry is still answered
    edge = np.array([[0.0, 0.0, 0.0], [16383.5, 16383.5, 1.0]])
    assert alg.pmf_grid(make_buffer(hip, edge, "H"), 1.0)["cols"] == 1 << 14
    assert _code(lambda: alg.pmf_grid(make_buffer(hip, edge + [[0, 0, 0], [1.0, 0, 0]], "H"), 1.0)) == 23
    # and the next call works
    mask, count = alg.ground_mask(buf, alg.PmfParameters(100.0, 3000.0))
    assert mask.tolist() == [1, 1] and count == 2
    check(hip, terrain(500, 50), SCENE_PARAMS, what="after the refusals")


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/classify_ground.py: rolling terrain is classified, the boxes and poles come out as clusters, and a single plane does worse."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("classify_ground", os.path.join(root, "examples", "classify_ground.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(60000)
    assert result["ground_recall"] >= 0.99 and result["objects_as_ground"] == 0
    assert result["clusters_found"] == result["objects_planted"]
    assert result["plane_left_over"] > 10 * result["pmf_left_over"]
