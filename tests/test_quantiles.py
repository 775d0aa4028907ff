"""pst_rasterize_quantiles and pst_segment_quantiles against tests/quantiles_ref.py, the numpy restatement of the header's definition.

Selection is exact: every comparison is of u64 views, without a tolerance.  The CPU tests pin the restatement itself (a hand-computed table,
numpy's own quantile, the knife edges of g) and the argument checks; the GPU tests place group sizes, group boundaries and point counts at
the seams of the kernels (pst_quantiles_kernel_shape)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import quantiles_ref as Q
import raster_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS_PER_BLOCK = 1536  # asserted against pst_quantiles_kernel_shape below: the parametrisations need them at collection time
CAP = 512
WINDOW = 2048
KEY_BLOCK = 256  # points per workgroup of the key and gather kernels (raster.hip, segments.hip)
NONE = 0xFFFFFFFF
INF = float("inf")
PROBS = (0.0, 0.25, 0.5, 0.95, 1.0)
THRESHOLDS = (0.0, 1e3)
GROUP_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, CAP - 1, CAP, CAP + 1, 2 * CAP + 1, 200_003]
SEAM_LENGTHS = [1, 2, 63, 64, 65, KEY_BLOCK - 1, KEY_BLOCK, KEY_BLOCK + 1, POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, WINDOW - 1, WINDOW, WINDOW + 1,
                3 * POINTS_PER_BLOCK + 5, 65535, 65536, 65537]
# the tests a child process repeats with every group on the general path (PST_QUANTILES_GENERAL=1)
GENERAL_PATH_TESTS = "test_group_sizes or test_packing or test_values_zeros_denormals_and_overflow or test_parameters"


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _empty_buffer(hip, dtype=T.Vec3f64):
    return HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _dev(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)  # (an address that is not NULL; nothing of it is read)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).cuda()


def _doubles(values):
    return (C.c_double * max(len(values), 1))(*values), len(values)


def _run(call, planes, groups, device_out):
    """the planes [planes][groups] a call wrote, through host memory or through device memory between guard entries"""
    if device_out:
        import torch
        d = torch.full((planes * groups + 2,), 123.0, dtype=torch.float64, device="cuda")
        call(C.c_void_p(d.data_ptr() + 8), 0)
        d = d.cpu().numpy()
        assert d[0] == 123.0 and d[-1] == 123.0, "a guard entry around the device results was written"
        return d[1:-1].reshape(planes, groups).copy()
    out = np.full((planes, groups), 5.0)
    call(C.c_void_p(out.ctypes.data if out.size else 1), 1)
    return out


def gpu_segments(hip, pts, labels, S, probs=PROBS, thresholds=THRESHOLDS, method="linear", values=None, mask=None, storage="H", device_out=False):
    """-> (planes [1 + P + T][S], n_members) through the C ABI; labels, values and mask go through device memory"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip)
    dl = _dev((np.asarray(labels).astype(np.int64) & NONE).astype(np.uint32), np.uint32)
    dv = _dev(values, np.float64) if values is not None else None
    dm = _dev(mask, np.uint8) if mask is not None else None
    (p, P), (t, Tn) = _doubles(probs), _doubles(thresholds)
    members = C.c_uint64(99)
    out = _run(lambda dst, kind: hip.segment_quantiles(buf._h, C.c_void_p(dl.data_ptr()), S, C.c_void_p(dv.data_ptr()) if dv is not None else None,
                                                       C.c_void_p(dm.data_ptr()) if dm is not None else None, p, P, Q.METHODS[method], t, Tn, dst, kind, C.byref(members)),
               1 + P + Tn, S, device_out)
    return out, members.value


def gpu_raster(hip, pts, cell, probs=PROBS, thresholds=THRESHOLDS, method="linear", values=None, mask=None, origin=None, dim=None, storage="H", device_out=False):
    """-> (planes [1 + P + T][rows * cols], n_members, (x0, y0, cols, rows)) through the C ABI; the automatic grid is sized by the restatement"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    buf = make_buffer(hip, pts, storage) if len(pts) else _empty_buffer(hip)
    dv = _dev(values, np.float64) if values is not None else None
    dm = _dev(mask, np.uint8) if mask is not None else None
    (p, P), (t, Tn) = _doubles(probs), _doubles(thresholds)
    cols, rows = dim if dim is not None else R.auto_grid(pts, cell)[2:]
    c_origin = (C.c_double * 2)(*origin) if origin is not None else None
    c_dim = (C.c_uint32 * 2)(*dim) if dim is not None else None
    origin_out, dim_out, members = (C.c_double * 2)(7.0, 7.0), (C.c_uint32 * 2)(7, 7), C.c_uint64(99)
    out = _run(lambda dst, kind: hip.rasterize_quantiles(buf._h, C.c_void_p(dv.data_ptr()) if dv is not None else None, C.c_void_p(dm.data_ptr()) if dm is not None else None,
                                                         cell, c_origin, c_dim, p, P, Q.METHODS[method], t, Tn, dst, kind, origin_out, dim_out, C.byref(members)),
               1 + P + Tn, cols * rows, device_out)
    return out, members.value, (origin_out[0], origin_out[1], dim_out[0], dim_out[1])


def assert_planes(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(Q.bits(got) != Q.bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first (plane, group) {bad[:3].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def cloud_of(group, values, cols, seed=0):
    """points whose cell on the grid of origin (0, 0), cell size 1 and `cols` columns is `group`, z = values, in a shuffled order;
    -> (pts, labels): the same multiset of (group, value) through either entry point"""
    group = np.asarray(group, dtype=np.int64)
    rng = np.random.default_rng([seed, len(group)])
    pts = np.column_stack([group % cols + rng.uniform(0.1, 0.9, len(group)), group // cols + rng.uniform(0.1, 0.9, len(group)), np.asarray(values, dtype=np.float64)])
    order = rng.permutation(len(group))
    return pts[order], group[order]


def check_groups(hip, group, values, G, probs=PROBS, thresholds=THRESHOLDS, method="linear", what="", entries=("segments", "raster"), **kw):
    """the multiset of (group, value) through both entry points, against the core of the restatement"""
    want = Q.group_planes(group, values, G, probs, thresholds, method)
    cols = max(1, min(G, 1000))
    rows = -(-G // cols)
    pts, labels = cloud_of(group, values, cols)
    if "segments" in entries:
        got, members = gpu_segments(hip, pts, labels, G, probs, thresholds, method, **kw)
        assert_planes(got, want, what + " segments")
        assert members == len(labels)
    if "raster" in entries:
        got, members, grid = gpu_raster(hip, pts, 1.0, probs, thresholds, method, origin=(0.0, 0.0), dim=(cols, rows), **kw)
        assert_planes(got[:, :G], want, what + " raster")
        assert members == len(labels) and grid == (0.0, 0.0, cols, rows)
    return want


def groups_of_sizes(sizes):
    """group ids: group g has sizes[g] members"""
    return np.repeat(np.arange(len(sizes)), sizes)


# ------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_restatement_on_a_hand_computed_table():
    """Three segments, the middle one empty; a pair of zeros; a non-member of every kind; the three methods; thresholds at a member's value,
    at 0.0 and at -0.0.  Every expected number below was worked out by hand from the header's text."""
    nan = np.nan
    pts = np.array([[0, 0, 3.0], [0, 0, -0.0], [0, 0, 0.0], [0, 0, 1.0],  # segment 0: sorted -0.0, +0.0, 1.0, 3.0
                    [0, 0, 5.0], [0, 0, 2.0],                              # segment 2: sorted 2.0, 5.0
                    [0, 0, 9.0], [0, 0, 9.0], [0, 0, nan], [INF, 0, 9.0], [0, 0, 9.0], [0, 0, 9.0]])
    labels = np.array([0, 0, 0, 0, 2, 2, 7, NONE, 0, 0, 0, 2])  # label >= S, no label, NaN value, inf coordinate, masked out (twice)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], dtype=np.uint8)
    probs, thresholds = (0.0, 0.25, 0.5, 1.0), (1.0, 0.0, -0.0)
    # p = 0.25, m = 4: h = 0.75, lo = 0, g = 0.75: -0.0 + 0.75 * (0.0 - -0.0) = +0.0;  p = 0.5: h = 1.5, lo = 1: 0.0 + 0.5 * (1.0 - 0.0)
    # m = 2: p = 0.25: 2 + 0.25 * 3 = 2.75;  p = 0.5: 3.5
    expect = {
        "linear": [[-0.0, nan, 2.0], [0.0, nan, 2.75], [0.5, nan, 3.5], [3.0, nan, 5.0]],
        "lower": [[-0.0, nan, 2.0], [-0.0, nan, 2.0], [0.0, nan, 2.0], [3.0, nan, 5.0]],
        "higher": [[-0.0, nan, 2.0], [0.0, nan, 5.0], [1.0, nan, 5.0], [3.0, nan, 5.0]],
    }
    above = [[1.0, 0.0, 2.0], [2.0, 0.0, 2.0], [2.0, 0.0, 2.0]]  # > 1.0: {3.0}; > 0.0 and > -0.0: {1.0, 3.0} -- neither zero is above the other
    for method, rows in expect.items():
        got, members = Q.segment_quantiles(pts, labels, 3, probs, thresholds, method, mask=mask)
        want = np.array([[4.0, 0.0, 2.0]] + rows + above)
        want[np.isnan(want)] = Q.NAN
        assert_planes(got, want, method)
        assert members == 6
    # the same multiset through the raster's restatement: three cells in a row, the non-members outside, not finite or masked
    cells = np.array([[0.5, 0.5, 3.0], [0.5, 0.5, -0.0], [0.5, 0.5, 0.0], [0.5, 0.5, 1.0], [2.5, 0.5, 5.0], [2.5, 0.5, 2.0],
                      [3.0, 0.5, 9.0], [-1e-9, 0.5, 9.0], [0.5, 0.5, nan], [nan, 0.5, 9.0], [0.5, 0.5, 9.0], [2.5, 0.5, 9.0]])
    got, members, grid = Q.rasterize_quantiles(cells, 1.0, probs, thresholds, "linear", mask=mask, origin=(0.0, 0.0), dim=(3, 1))
    want = np.array([[4.0, 0.0, 2.0]] + expect["linear"] + above)
    want[np.isnan(want)] = Q.NAN
    assert_planes(got, want, "raster")
    assert members == 6 and grid == (0.0, 0.0, 3, 1)


@pytest.mark.parametrize("m", [1, 2, 5, 64, 1000, 4097])
def test_restatement_against_numpy(m):
    """np.quantile's 'lower' and 'higher' bit for bit (a cloud without zeros of mixed sign), 'linear' within a few ulp: numpy interpolates
    with another expression of the same h"""
    v = R.wide_values(m, m)
    s = Q.sort_values(v)
    assert np.array_equal(s, np.sort(v))
    probs = np.concatenate([[0.0, 1.0, 0.5, 0.95], np.random.default_rng(m).random(40)])
    for p in probs:
        for method in ("lower", "higher"):
            assert Q.bits(Q.quantile(s, p, method)) == Q.bits(np.quantile(v, p, method=method)), (p, method)
        # with M the larger magnitude of the two neighbours: the difference (up to 2 M) rounds by at most ulp(M), its product with g < 1 and
        # the final sum by as much each -- 3 ulp(M) per expression, 6 between two of them (the values have mixed signs: the RESULT may be tiny)
        got, want = Q.quantile(s, p), np.quantile(v, p, method="linear")
        lo = int(np.floor(np.float64(m - 1) * p))
        big = max(abs(s[lo]), abs(s[min(lo + 1, m - 1)]))
        assert abs(got - want) <= 6 * np.spacing(big), (p, got, want)
    assert Q.bits(Q.quantile(s, 0.0)) == Q.bits(s[0]) and Q.bits(Q.quantile(s, 1.0)) == Q.bits(s[-1])


def test_restatement_sorts_the_zeros_by_their_sign():
    v = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0])
    assert Q.bits(Q.sort_values(v)).tolist() == [1 << 63] * 3 + [0] * 3
    assert Q.bits(np.sort(v)).tolist() != Q.bits(Q.sort_values(v)).tolist()  # (np.sort leaves them as they came: why it is not used)


def test_knife_edges_of_g():
    """m - 1 a power of two and p = j / (m - 1): g is exactly 0 and the result has a member's bits.  One ulp beside it: interpolated."""
    m = 65
    s = Q.sort_values(R.wide_values(m, 3))
    for j in range(m):
        p = j / (m - 1)
        for method in Q.METHODS:
            assert Q.bits(Q.quantile(s, p, method)) == Q.bits(s[j]), (j, method)
        if j < m - 1:
            up = np.nextafter(p, 2.0)
            assert Q.bits(Q.quantile(s, up, "lower")) == Q.bits(s[j]) and Q.bits(Q.quantile(s, up, "higher")) == Q.bits(s[j + 1])
            g = np.float64(m - 1) * up - j
            assert g > 0.0 and Q.bits(Q.quantile(s, up)) == Q.bits(s[j] + g * (s[j + 1] - s[j]))
        if j > 0:
            down = np.nextafter(p, -1.0)
            assert Q.bits(Q.quantile(s, down, "lower")) == Q.bits(s[j - 1]) and Q.bits(Q.quantile(s, down, "higher")) == Q.bits(s[j])
            g = np.float64(m - 1) * down - (j - 1)
            assert 0.0 < g < 1.0 and Q.bits(Q.quantile(s, down)) == Q.bits(s[j - 1] + g * (s[j] - s[j - 1]))


def test_kernel_shape(hip):
    assert alg.quantiles_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK, "cap": CAP, "window": WINDOW}
    assert POINTS_PER_BLOCK + CAP - 1 <= WINDOW  # a small group that starts in a workgroup's positions ends inside its window
    one = C.c_uint32(7)
    hip.quantiles_kernel_shape(None, C.byref(one), None)  # each pointer is optional
    assert one.value == CAP
    hip.quantiles_kernel_shape(None, None, None)
    assert alg.quantiles_phase_times(hip) == (0.0, 0.0, 0.0, 0.0)
    assert _code(lambda: hip.quantiles_phase_times(None)) == 1


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments, invalid parameters and a missing position: the same answer with or without a device, because none is looked for."""
    buf, f32 = _empty_buffer(hip), _empty_buffer(hip, T.Vec3f32)
    out, members = (C.c_double * 32)(*([5.0] * 32)), C.c_uint64(9)
    labels = C.c_void_p(8)  # (never read: every call below is refused first)
    half, (t0, _) = _doubles([0.5])[0], _doubles([2.0])
    below_zero, above_one = float(np.nextafter(-0.0, -1.0)), float(np.nextafter(1.0, 2.0))

    def seg(b=buf._h, lab=labels, S=2, probs=half, P=1, method=0, thr=t0, Tn=1, dst=out, kind=1, m=C.byref(members)):
        return lambda: hip.segment_quantiles(b, lab, S, None, None, probs, P, method, thr, Tn, dst, kind, m)

    def ras(b=buf._h, cell=1.0, origin=None, dim=None, probs=half, P=1, method=0, thr=t0, Tn=1, dst=out, kind=1, m=C.byref(members)):
        c_origin = (C.c_double * 2)(*origin) if origin is not None else None
        c_dim = (C.c_uint32 * 2)(*dim) if dim is not None else None
        return lambda: hip.rasterize_quantiles(b, None, None, cell, c_origin, c_dim, probs, P, method, thr, Tn, dst, kind, None, None, m)

    for call in (seg, ras):
        assert _code(call(b=None)) == 1 and _code(call(dst=None)) == 1 and _code(call(m=None)) == 1
        assert _code(call(kind=7)) == 1  # no such memory kind
        for bad in (float("nan"), below_zero, above_one, -1.0, 2.0, INF):
            assert _code(call(probs=_doubles([0.5, bad])[0], P=2)) == 1, bad
        assert _code(call(thr=_doubles([float("nan")])[0])) == 1
        for method in (3, 4, 1 << 31):
            assert _code(call(method=method)) == 1
        assert _code(call(P=0, Tn=0)) == 1  # no plane
        many = _doubles([0.5] * 65)[0]
        assert _code(call(probs=many, P=65, Tn=0)) == 1 and _code(call(thr=many, P=0, Tn=65)) == 1 and _code(call(probs=many, P=64, thr=many, Tn=1)) == 1
        assert _code(call(probs=None)) == 1 and _code(call(thr=None)) == 1  # an array of one entry that is not there
        # a position that is not Vec3f64 is known from the layout alone -- and is looked at AFTER the parameters
        assert _code(call(b=f32._h)) == 4 and _code(call(b=f32._h, method=3)) == 1 and _code(call(b=f32._h, P=0, Tn=0)) == 1
        with pytest.raises(PasturePanic):
            call(b=f32._h)()
    assert _code(seg(lab=None)) == 1 and _code(seg(S=0)) == 1 and _code(seg(b=f32._h, S=0)) == 1
    for cell in (0.0, -1.0, INF, float("nan")):
        assert _code(ras(cell=cell)) == 1
    assert _code(ras(origin=(0.0, 0.0))) == 1 and _code(ras(dim=(2, 2))) == 1  # together or not at all
    assert _code(ras(origin=(INF, 0.0), dim=(2, 2))) == 1 and _code(ras(origin=(0.0, 0.0), dim=(0, 2))) == 1
    assert _code(ras(origin=(0.0, 0.0), dim=(1 << 14, (1 << 14) + 1))) == 23  # more than 2^28 cells
    # legal edges: an empty buffer on the automatic grid is answered on the host, with nothing written
    members.value = 9
    hip.rasterize_quantiles(buf._h, None, None, 1.0, None, None, _doubles([0.0, -0.0, 1.0])[0], 3, 2, _doubles([INF, -INF])[0], 2, out, 1, None, None, C.byref(members))
    assert members.value == 0 and list(out) == [5.0] * 32
    with pytest.raises(ValueError):
        alg.rasterize_quantiles(buf, 1.0, method="nearest")
    with pytest.raises(ValueError):
        alg.segment_quantiles(buf, np.zeros(3, dtype=np.uint32), 2)  # three labels for no points


def test_no_device_is_an_error_not_a_cpu_path(hip):
    import torch
    if torch.cuda.is_available():
        return  # (with a device these calls are the GPU tests below)
    buf = _empty_buffer(hip)
    out, members = (C.c_double * 8)(), C.c_uint64()
    p, t = _doubles([0.5])[0], _doubles([2.0])[0]
    assert _code(lambda: hip.segment_quantiles(buf._h, C.c_void_p(8), 2, None, None, p, 1, 0, t, 1, out, 1, C.byref(members))) == 21
    assert _code(lambda: hip.rasterize_quantiles(buf._h, None, None, 1.0, (C.c_double * 2)(0, 0), (C.c_uint32 * 2)(2, 2), p, 1, 0, t, 1, out, 1, None, None, C.byref(members))) == 21


# ------------------------------------------------------------------------------------------------------------------------------ the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("m", GROUP_SIZES)
def test_group_sizes(hip, m):
    """one group of m members between two small ones and three empty ones, through both entry points; wide values, so that an
    interpolation shows a wrong neighbour"""
    group = groups_of_sizes([0, 7, 0, m, 5, 0])
    check_groups(hip, group, R.wide_values(len(group), m), 6, what=f"m={m}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["singles", "ramp", "empty_runs", "heavy_between", "two_heavy", "one_group"])
def test_packing(hip, case):
    sizes = {
        "singles": [1] * 70_001,                                      # a workgroup packs points_per_block groups
        "ramp": list(range(1, 301)),                                  # boundaries on every lane, wave and workgroup seam
        "empty_runs": [0] * 5 + [3, 0, 0, 9, 1] + [0] * 700 + [CAP, 2] + [0] * 2000 + [40] * 50 + [0] * 3,
        "heavy_between": [10] * 200 + [CAP + 300] + [10] * 200,       # a large group between small ones, across a window's end
        "two_heavy": [4, CAP + 1, 3 * CAP + 7, 4],
        "one_group": [20_011],
    }[case]
    group = groups_of_sizes(sizes)
    check_groups(hip, group, R.wide_values(len(group), 5), len(sizes), what=case)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0] + SEAM_LENGTHS)
def test_point_count_seams(hip, n):
    """n points over 40 groups with every fifth point a non-member, through host and device output"""
    rng = np.random.default_rng([4, n])
    group, values = rng.integers(0, 40, n), R.wide_values(n, n + 1)
    labels = np.where(np.arange(n) % 5 == 4, NONE, group)
    pts = np.column_stack([rng.random((n, 2)) * 8.0, values])
    want, members = Q.segment_quantiles(pts, labels, 40, PROBS, THRESHOLDS)
    for device_out in (False, True):
        got = gpu_segments(hip, pts, labels, 40, device_out=device_out)
        assert_planes(got[0], want, f"n={n}")
        assert got[1] == members
    want, members, grid = Q.rasterize_quantiles(pts, 1.0, PROBS, THRESHOLDS, origin=(0.0, 0.0), dim=(8, 7))
    got = gpu_raster(hip, pts, 1.0, origin=(0.0, 0.0), dim=(8, 7), device_out=True)
    assert_planes(got[0], want, f"raster n={n}")
    assert got[1:] == (members, grid)


@pytest.mark.gpu
def test_values_zeros_denormals_and_overflow(hip):
    sizes = [9, 300, CAP + 9]
    group = groups_of_sizes(sizes)
    n = len(group)
    rng = np.random.default_rng(8)
    probs, thr = (0.0, 0.5, 1.0, 0.3, 0.77), (0.0, -0.0, 5e-324, 1.7e308, -1.7e308)
    check_groups(hip, group, np.full(n, 2.5), 3, probs, (2.5, 2.0), what="all equal")
    check_groups(hip, group, rng.integers(0, 4, n).astype(np.float64), 3, probs, (0.0, 1.0, 2.0, 3.0), what="duplicates")
    # the lower half of every group -0.0, the upper half +0.0 (odd sizes: one more -0.0): p = 0 is -0.0, p = 1 is +0.0, and no zero is above a zero
    zeros = np.concatenate([np.where(np.arange(m) < (m + 1) // 2, -0.0, 0.0) for m in sizes])
    for method in Q.METHODS:
        want = check_groups(hip, group, zeros, 3, (0.0, 0.5, 1.0), (0.0, -0.0), method, what="zeros " + method)
        assert Q.bits(want[1]).tolist() == [1 << 63] * 3 and Q.bits(want[3]).tolist() == [0] * 3 and not want[4:].any()
    check_groups(hip, group, rng.integers(-3, 4, n) * 5e-324, 3, probs, thr, what="denormals")
    # the difference of neighbours overflows: IEEE is the definition
    halves = np.concatenate([np.where(np.arange(m) < m // 2, -1.7e308, 1.7e308) for m in sizes])  # s_lo < 0 < s_(lo+1) at h in (m // 2 - 1, m // 2)
    want = check_groups(hip, group, halves, 3, (0.0, 0.45, 0.499, 0.5, 1.0), thr, what="overflow")
    assert np.isinf(want[2, 0]) and np.isinf(want[3, 2]) and np.isinf(want[4, 1])  # 8 * 0.45 = 3.6, 520 * 0.499 = 259.48, 299 * 0.5 = 149.5


@pytest.mark.gpu
def test_members(hip):
    """a value column against z, values and coordinates that are not finite, the masks, labels that name no segment"""
    n, S = 5000, 7
    rng = np.random.default_rng(2)
    pts = np.column_stack([rng.random((n, 2)) * 6.0, R.wide_values(n, 1)])
    values = R.wide_values(n, 2)
    labels = rng.integers(0, S + 2, n)
    labels[::17] = NONE
    for a in (pts[:, 0], pts[:, 1], pts[:, 2], values):
        a[rng.integers(0, n, 40)] = rng.choice([np.nan, INF, -INF], 40)
    masks = {"none": None, "all": np.ones(n, dtype=np.uint8), "nothing": np.zeros(n, dtype=np.uint8), "every other": (np.arange(n) % 2 * 200).astype(np.uint8)}
    for name, mask in masks.items():
        for vals in (None, values):
            what = f"mask {name}, {'z' if vals is None else 'values'}"
            want, members = Q.segment_quantiles(pts, labels, S, PROBS, THRESHOLDS, values=vals, mask=mask)
            got = gpu_segments(hip, pts, labels, S, values=vals, mask=mask)
            assert_planes(got[0], want, what)
            assert got[1] == members
            want, members, grid = Q.rasterize_quantiles(pts, 0.75, PROBS, THRESHOLDS, values=vals, mask=mask)
            got = gpu_raster(hip, pts, 0.75, values=vals, mask=mask)
            assert_planes(got[0], want, what + " raster")
            assert got[1:] == (members, grid)
            assert grid == R.auto_grid(pts, 0.75)  # whatever the mask


@pytest.mark.gpu
@pytest.mark.parametrize("method", list(Q.METHODS))
def test_parameters(hip, method):
    sizes = [1, 2, 33, 0, CAP, CAP + 40]
    group = groups_of_sizes(sizes)
    values = R.wide_values(len(group), 6)
    values[::9] = 0.0
    values[4::9] = -0.0
    rng = np.random.default_rng(12)
    member = float(values[50])
    for probs, thr in [((0.95,), (member,)), (tuple(np.linspace(0.05, 0.95, 19)), (2.0,)), (tuple(rng.random(63)), (0.0,)), ((), (member, 0.0, -0.0, INF, -INF)),
                       ((0.9, 0.1, 0.5, 0.5, 1.0, 0.0, 0.1), ()), ((0.5,), (-0.0,)), ((0.5,), (0.0,))]:
        check_groups(hip, group, values, len(sizes), probs, thr, method, what=f"{len(probs)} probs, {len(thr)} thresholds, {method}")


@pytest.mark.gpu
def test_against_rasterize_and_segment_statistics(hip):
    """p = 0 and p = 1 are the MIN and MAX planes of the existing calls bit for bit, and the COUNT planes and n_members are theirs"""
    n, S = 30_000, 50
    rng = np.random.default_rng(21)
    pts = np.column_stack([rng.random((n, 2)) * 20.0, R.wide_values(n, 3)])
    pts[::7, 2] = np.where(rng.random(len(pts[::7])) < 0.5, -0.0, 0.0)
    labels = rng.integers(0, S + 5, n)
    labels[rng.random(n) < 0.6] = 3  # one segment above the cap
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    buf = make_buffer(hip, pts, "H")
    for m in (None, mask):
        q = alg.segment_quantiles(buf, labels, S, probs=(0.0, 1.0), mask=m)
        t = alg.segment_statistics(buf, labels, S, ("count", "value_min", "value_max"), mask=m)
        assert np.array_equal(Q.bits(q.count), Q.bits(t.count)) and q.n_members == t.n_members and q.count[3] > CAP
        assert np.array_equal(Q.bits(q.quantiles[0]), Q.bits(t.value_min)) and np.array_equal(Q.bits(q.quantiles[1]), Q.bits(t.value_max))
        dm = _dev(m, np.uint8) if m is not None else None
        for cell in (0.5, 10.0):  # 19 points per cell; 7500: large groups
            rq = alg.rasterize_quantiles(buf, cell, probs=(0.0, 1.0), device_mask_ptr=dm.data_ptr() if dm is not None else None)
            rs = alg.rasterize(buf, cell, ("count", "min", "max"), device_mask_ptr=dm.data_ptr() if dm is not None else None)
            assert (rq.origin, rq.cols, rq.rows, rq.n_members) == (rs.origin, rs.cols, rs.rows, rs.n_members)
            grid = alg.pmf_grid(buf, cell)
            assert (rq.origin, rq.cols, rq.rows) == (grid["origin"], grid["cols"], grid["rows"])
            assert rq.planes["count"].shape == (rs.rows, rs.cols) and rq.planes["quantiles"].shape == (2, rs.rows, rs.cols) and rq.planes["above"].shape == (0, rs.rows, rs.cols)
            assert np.array_equal(Q.bits(rq.planes["count"]), Q.bits(rs.planes["count"]))
            assert np.array_equal(Q.bits(rq.planes["quantiles"][0]), Q.bits(rs.planes["min"])) and np.array_equal(Q.bits(rq.planes["quantiles"][1]), Q.bits(rs.planes["max"]))


@pytest.mark.gpu
def test_invariance(hip):
    """the same bytes for the cloud shuffled, in H and V storage (and packed, sliced, external), through host and device output, twice"""
    sizes = [3, 0, 700, 41, CAP, CAP + 1, 1, 1, 90]
    group = groups_of_sizes(sizes)
    n, S = len(group), len(sizes)
    pts, labels = cloud_of(group, R.wide_values(n, 13), 3)
    first = gpu_segments(hip, pts, labels, S)
    first_raster = gpu_raster(hip, pts, 1.0, origin=(0.0, 0.0), dim=(3, 3))
    assert_planes(first[0], Q.group_planes(group, R.wide_values(n, 13), S, PROBS, THRESHOLDS), "the cloud itself")
    rng = np.random.default_rng(0)
    runs = [("again", np.arange(n), "H", False), ("shuffled", rng.permutation(n), "H", False), ("reversed", np.arange(n)[::-1], "H", True), ("V", np.arange(n), "V", False),
            ("device", np.arange(n), "V", True), ("packedH", rng.permutation(n), "packedH", False), ("slicepackedV", np.arange(n), "slicepackedV", True),
            ("external", rng.permutation(n), "external", False)]
    for what, order, storage, device_out in runs:
        got = gpu_segments(hip, pts[order], labels[order], S, storage=storage, device_out=device_out)
        assert got[0].tobytes() == first[0].tobytes() and got[1] == first[1], what
        got = gpu_raster(hip, pts[order], 1.0, origin=(0.0, 0.0), dim=(3, 3), storage=storage, device_out=device_out)
        assert got[0].tobytes() == first_raster[0].tobytes() and got[1:] == first_raster[1:], what


@pytest.mark.gpu
def test_general_path_forced_on_every_group():
    """PST_QUANTILES_GENERAL=1: every group takes the two radix sorts.  The group-size, packing, value and parameter tests again, against
    the same restatement -- so the planes are the LDS path's byte for byte.  The switch is read once per process, hence the child
    interpreter."""
    env = dict(os.environ, PST_QUANTILES_GENERAL="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_quantiles.py"), "-x", "-q", "-m", "gpu", "-k", GENERAL_PATH_TESTS,
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    passed = re.search(r"(\d+) passed", r.stdout)
    assert passed and int(passed.group(1)) == len(GROUP_SIZES) + 6 + 1 + len(Q.METHODS) and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]


@pytest.fixture(scope="module")
def forest():
    """200 003 points of test_trees.py's stand with real heights, and a tree label per point: the nearest trunk within 4 m"""
    from test_trees import stand
    pts, trunks, heights = stand(200_003, 17, 120.0, noise=0.05)
    labels = np.full(len(pts), NONE, dtype=np.int64)
    for c0 in range(0, len(pts), 20000):
        d2 = ((pts[c0:c0 + 20000, None, :2] - trunks[None, :, :]) ** 2).sum(axis=2)
        near = d2.argmin(axis=1)
        labels[c0:c0 + 20000] = np.where(d2[np.arange(len(near)), near] <= 16.0, near, NONE)
    return pts, labels, len(trunks), heights


@pytest.mark.gpu
def test_a_forest(hip, forest):
    """the larger case: p50 and p95 of the heights and the returns above 2 m, per 10 m cell and per tree, exactly; and through the Python calls"""
    pts, labels, S, heights = forest
    probs, thr = (0.5, 0.95), (2.0,)
    want, members, grid = Q.rasterize_quantiles(pts, 10.0, probs, thr)
    buf = make_buffer(hip, pts, "H")
    r = alg.rasterize_quantiles(buf, 10.0, probs, thr)
    assert (r.origin[0], r.origin[1], r.cols, r.rows) == grid and r.n_members == members
    got = np.concatenate([r.planes["count"][None], r.planes["quantiles"], r.planes["above"]]).reshape(4, -1)
    assert_planes(got, want, "raster")
    assert np.median(got[0]) > CAP  # the cells took the large-group path ...
    want, members = Q.segment_quantiles(pts, labels, S, probs, thr)
    q = alg.segment_quantiles(buf, labels, S, probs, thr)
    assert_planes(np.concatenate([q.count[None], q.quantiles, q.above]), want, "trees")
    assert q.n_members == members and 0 < q.count.min() and q.count.max() > CAP  # ... and the crowns both
    assert np.array_equal(q.cover(0), q.above[0] / q.count)
    # a tree's p95 stays below the height it was planted with, and not far below (paraboloid crowns: few returns near the apex)
    assert (q.quantiles[1] < heights + 0.5).all() and (q.quantiles[1] > 0.5 * heights).all()
    fine = alg.rasterize_quantiles(buf, 0.5, probs, thr)  # 3.5 points per cell: every cell on the LDS path
    want, members, grid = Q.rasterize_quantiles(pts, 0.5, probs, thr)
    got = np.concatenate([fine.planes["count"][None], fine.planes["quantiles"], fine.planes["above"]]).reshape(4, -1)
    assert_planes(got, want, "fine raster")
    assert got[0].max() <= CAP and fine.n_members == members


@pytest.mark.gpu
def test_forest_metrics_example():
    """examples/forest_metrics.py: a crown is a paraboloid of radius H / 4 labelled out to 0.3 H from its top and down to 0.3 H, so 5 % of
    its labelled area lies above H * (1 - 0.05 * 0.7) = 0.965 H: the p95 of every tree sits a little under the height it was planted
    with (the height above ground is interpolated over rolling terrain: half a metre of room), never above the tree's largest height."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("forest_metrics", os.path.join(ROOT, "examples", "forest_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = mod.metrics(60_000, 3)
    assert len(m["trees"]) >= m["planted"] - 2
    for t, p95, top, planted, count in m["trees"]:
        assert 0.85 * planted < p95 <= top <= planted + 0.5, (t, p95, top, planted, count)
    stand = m["in_stand"]
    assert stand.sum() == 36 and (m["p50"][stand] <= m["p95"][stand]).all() and (m["p95"][stand] > 5.0).all()
    assert ((m["cover"][stand] > 0.1) & (m["cover"][stand] < 0.9)).all()  # crowns of radius 2 - 5 m on a 10 m lattice: neither bare nor closed
