"""M3C2 change detection (pst_m3c2_device, pst_m3c2_kernel_shape, pst_m3c2_phase_times, pst_m3c2_work) against tests/m3c2_ref.py.

CPU tests pin the restatement on hand-built cases with known answers and check every refusal that is answered on the host.  GPU tests compare
the HIP kernel with the restatement: counts equal, unit normals bit for bit, the two sums per cloud within 2 * m * 2^-53 * sum |term| of the
fsum value (m members: the worst case of ANY order of summation, times two -- the bound of test_nearest.test_icp_step_sums; the terms are the same
bits on both sides), and distance, lod and significance bit for bit the header's formulas applied in numpy to the device's OWN counts and sums.
Every device result is computed twice and the two calls must agree in every bit."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import m3c2_ref as M
import nn_ref
from harness import make_buffer as layout_buffer
from pasture_amd import PastureError
from pasture_amd import algorithms as alg
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_nearest import _code, _empty_buffer, bits, buffer_of, lattice, reference

CORES = 4                # core points per workgroup and lanes per core point; asserted against pst_m3c2_kernel_shape: the parametrisations need
LANES = 64               # them at collection time
EPS = 2.0 ** -53
INF = float("inf")
NAN = float("nan")
UP = np.array([0.0, 0.0, 1.0])


# ------------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def plane(n_side, z, spacing=0.25, origin=(-2.0, -2.0)):
    g = np.arange(n_side, dtype=np.float64) * spacing
    x, y = np.meshgrid(g + origin[0], g + origin[1], indexing="ij")
    return np.column_stack([x.ravel(), y.ravel(), np.full(x.size, z)])


def test_restatement_two_parallel_planes():
    """Two planes 0.5 apart, vertical normal: every member of plane 1 has t = 0 and of plane 2 t = 0.5, exactly; the disk of radius 0.5 around a
    lattice point of spacing 0.25 holds 13 lattice points (0.5^2 on the rim is inclusive)."""
    p1, p2 = plane(17, 0.0), plane(17, 0.5)
    core = np.array([[0.0, 0.0, 0.0], [0.25, -0.5, 0.0]])
    r = M.m3c2(core, p1, p2, 0.5, 1.0, normals=np.tile(UP, (2, 1)), min_points=4, registration_error=0.125)
    assert r["valid"].all() and np.array_equal(r["u"], np.tile(UP, (2, 1)))
    assert np.array_equal(r["counts"], [[13, 13], [13, 13]])
    assert np.array_equal(r["sums"], [[0.0, 0.0, 6.5, 3.25]] * 2)
    assert np.array_equal(r["distance"], [0.5, 0.5])
    assert np.array_equal(r["lod"], [1.96 * 0.125] * 2) and r["significant"].all()       # both spreads are 0
    # a registration error the distance does not exceed; the depth too short to reach plane 2; more points asked for than there are
    assert not M.m3c2(core, p1, p2, 0.5, 1.0, normals=np.tile(UP, (2, 1)), registration_error=0.5)["significant"].any()
    short = M.m3c2(core, p1, p2, 0.5, 0.25, normals=np.tile(UP, (2, 1)))
    assert np.array_equal(short["counts"], [[13, 0]] * 2) and np.isnan(short["distance"]).all() and not short["significant"].any()
    assert np.isnan(M.m3c2(core, p1, p2, 0.5, 1.0, normals=np.tile(UP, (2, 1)), min_points=14)["lod"]).all()
    # the sign: the same clouds swapped, and the normal turned over
    assert np.array_equal(M.m3c2(core, p2, p1, 0.5, 1.0, normals=np.tile(UP, (2, 1)))["distance"], [-0.5, -0.5])
    assert np.array_equal(M.m3c2(core, p1, p2, 0.5, 1.0, normals=np.tile(-UP, (2, 1)))["distance"], [-0.5, -0.5])
    assert np.array_equal(M.m3c2(core, p1, p2, 0.5, 1.0, normals=np.tile(-UP, (2, 1)), flags=M.ORIENT_UP)["distance"], [0.5, 0.5])


def test_restatement_tilted_normal():
    """Normal (3, 0, 4): u = (0.6, 0, 0.8).  Points c + a*u + b*v with v = (0, 1, 0) have t = a and r = |b| up to a rounding."""
    c = np.array([1.0, 2.0, 3.0])
    u, v = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0])
    ab1 = [(0.0, 0.0), (0.5, 0.25), (-0.5, -0.25), (1.5, 0.0), (0.0, 0.75), (2.5, 0.0)]     # the last: beyond L = 2; (0, 0.75): beyond R = 0.5
    ab2 = [(1.0, 0.0), (1.25, 0.25), (0.75, -0.25), (1.0, 0.5)]
    cloud1 = np.array([c + a * u + b * v for a, b in ab1])
    cloud2 = np.array([c + a * u + b * v for a, b in ab2])
    r = M.m3c2(c[None], cloud1, cloud2, 0.5, 2.0, normals=[[3.0, 0.0, 4.0]], min_points=2)
    assert np.array_equal(r["u"], [u]) and np.array_equal(r["counts"], [[4, 4]])
    assert abs(r["sums"][0, 0] - 1.5) < 1e-14 and abs(r["sums"][0, 2] - 4.0) < 1e-14
    assert abs(r["distance"][0] - (1.0 - 0.375)) < 1e-14
    var1, var2 = np.var([0.0, 0.5, -0.5, 1.5], ddof=1), np.var([1.0, 1.25, 0.75, 1.0], ddof=1)
    assert abs(r["lod"][0] - 1.96 * np.sqrt(var1 / 4 + var2 / 4)) < 1e-13


def test_restatement_single_member_and_invalid_core_points():
    """One member on either side with min_points 1: the distance is reported, lod is NaN, nothing is significant.  Invalid core points: NaN u,
    zero counts, NaN results."""
    core = np.array([[0.0, 0.0, 0.0], [NAN, 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    normals = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, NAN, 1.0], [0.0, 0.0, 0.0], [1e-200, 0.0, 1e-200], [INF, 0.0, 0.0]])
    r = M.m3c2(core, [[0.0, 0.0, 0.25], [NAN, 0.0, 0.0]], [[0.0, 0.0, 0.75], [0.0, 0.0, INF]], 1.0, 1.0, normals=normals, min_points=1)
    assert list(r["valid"]) == [True] + [False] * 6
    assert np.array_equal(r["counts"][0], [1, 1]) and r["distance"][0] == 0.5 and np.isnan(r["lod"][0]) and not r["significant"].any()
    assert np.isnan(r["u"][1:]).all() and not r["counts"][1:].any() and not r["sums"][1:].any() and np.isnan(r["distance"][1:]).all()
    assert np.isnan(M.m3c2(core, [[0.0, 0.0, 0.25]], [[0.0, 0.0, 0.75]], 1.0, 1.0, normals=normals, min_points=2)["distance"]).all()
    # the nearest point's normal; no reference point: no nearest point
    near = M.m3c2([[0.1, 0.0, 0.0]], [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.1, 0.0, 0.5]], 1.0, 1.0, reference_normals=[[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], min_points=1)
    assert np.array_equal(near["u"], [[-0.0, -0.0, -1.0]]) and near["distance"][0] == -0.5
    assert not M.m3c2([[0.1, 0.0, 0.0]], np.zeros((0, 3)), [[0.1, 0.0, 0.5]], 1.0, 1.0, reference_normals=np.zeros((0, 3)))["valid"].any()


def test_orientation_rule_of_the_restatement():
    n = np.array([[0.0, 0.0, -1.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [1.0, 1.0, -1.0], [-1.0, -1.0, 1.0], [1.0, 0.0, 0.0]])
    u, valid = M.unit_normals(np.zeros((8, 3)), n, M.ORIENT_UP)
    flipped = np.array([True, True, True, True, False, True, False, False])
    plain, _ = M.unit_normals(np.zeros((8, 3)), n)
    assert valid.all() and np.array_equal(u, np.where(flipped[:, None], -plain, plain))


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _blank_index():
    """An index over an empty target, stood up on the host (every field of pst_nn_index zero: test_icp_plane._blank_index).  has_normals cannot
    be set from here: an index WITH normals needs a device."""
    block = (C.c_uint8 * 4096)()
    return block, C.c_void_p(C.addressof(block))


def _call(hip, ref, cmp, core, normals=C.c_void_p(8), radius=1.0, depth=1.0, min_points=4, reg=0.0, flags=0, outs=None, nsig=None):
    outs = [C.c_void_p(8)] * 6 if outs is None else outs
    return hip.m3c2_device(ref, cmp, core, normals, radius, depth, min_points, reg, flags, *outs, nsig)


def test_kernel_shape(hip):
    assert alg.m3c2_kernel_shape(hip) == {"cores_per_block": CORES, "lanes_per_core": LANES}
    hip.m3c2_kernel_shape(None, None)


def test_argument_refusals_answered_on_the_host(hip):
    """Every refusal of the header, with or without a device, because none is looked for; then the missing normals, status 4."""
    keep, blank = _blank_index()
    buf, f32 = _empty_buffer(hip), _empty_buffer(hip, T.Vec3f32)
    b = buf._h
    assert _code(lambda: _call(hip, None, blank, b)) == 1
    assert _code(lambda: _call(hip, blank, None, b)) == 1
    assert _code(lambda: _call(hip, blank, blank, None)) == 1
    for bad in (NAN, INF, -INF, 0.0, -0.0, -1.0):
        assert _code(lambda: _call(hip, blank, blank, b, radius=bad)) == 1
        assert _code(lambda: _call(hip, blank, blank, b, depth=bad)) == 1
    for bad in (NAN, INF, -INF, -1e-300):
        assert _code(lambda: _call(hip, blank, blank, b, reg=bad)) == 1
    assert _code(lambda: _call(hip, blank, blank, b, min_points=0)) == 1
    for bad in (2, 4, 0x80000000, 3):
        assert _code(lambda: _call(hip, blank, blank, b, flags=bad)) == 1
    assert _code(lambda: _call(hip, blank, blank, b, outs=[None] * 6, nsig=None)) == 1            # no output at all
    assert _code(lambda: _call(hip, blank, blank, f32._h)) == 4                                   # Position3D is not Vec3f64
    assert _code(lambda: _call(hip, blank, blank, b, normals=None)) == 4                          # the reference has no normals
    assert _code(lambda: _call(hip, blank, blank, b, normals=None, nsig=C.byref(C.c_uint64()))) == 4
    # the refusals come before the missing normals
    assert _code(lambda: _call(hip, blank, blank, b, normals=None, radius=NAN)) == 1
    assert _code(lambda: hip.m3c2_phase_times(None)) == 1
    assert _code(lambda: hip.m3c2_work(None)) == 1
    assert alg.m3c2_phase_times(hip) == (0.0, 0.0, 0.0) or os.environ.get("PST_M3C2_TIMES")
    del keep


def test_past_the_checks_the_device_is_looked_for(hip):
    """With normals given and every argument in order the call goes on to the device: PST_ERR_NO_DEVICE without one, never a CPU path; with
    one, an empty core buffer is answered with zero significant points."""
    import torch
    keep, blank = _blank_index()
    buf, nsig = _empty_buffer(hip), C.c_uint64(7)
    if torch.cuda.is_available():
        _call(hip, blank, blank, buf._h, nsig=C.byref(nsig))
        assert nsig.value == 0
    else:
        with pytest.raises(PastureError) as e:
            _call(hip, blank, blank, buf._h, nsig=C.byref(nsig))
        assert e.value.code == 21 and "no CPU fallback" in str(e.value)
    del keep


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

OUTPUTS = ("distance", "lod", "significant", "counts", "sums", "unit")


def core_buffer(hip, pts, storage="H"):
    """"V" / "H": interleaved / columnar through harness.make_buffer; the storages of test_outliers.make_buffer otherwise"""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    if len(pts) == 0:
        return _empty_buffer(hip)
    if storage in ("V", "H"):
        layout = PointLayout.from_attributes([A.POSITION_3D], api=hip)
        rec = np.zeros(len(pts), dtype=layout.numpy_record_dtype())
        rec[A.POSITION_3D.name()] = pts
        return layout_buffer(storage, layout, rec)
    return buffer_of(hip, pts, storage)


def index_of(hip, pts, edge=0.0, normals=None):
    index = alg.NearestNeighbourIndex(buffer_of(hip, pts), edge)
    if normals is not None:
        import torch
        d = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float64)).cuda()
        index.set_normals(d.data_ptr(), len(normals))
        torch.cuda.synchronize()
    return index


def auto_edge(hip, pts):
    index = index_of(hip, pts)
    try:
        return index.grid()["cell_edge"]
    finally:
        index.destroy()


def run_once(core, ref, cmp, radius, depth, normals, min_points, reg, orient, skip=()):
    import torch
    n = core.len()
    shapes = {"distance": ((n,), torch.float64), "lod": ((n,), torch.float64), "significant": ((n,), torch.uint8), "counts": ((n, 2), torch.int32),
              "sums": ((n, 4), torch.float64), "unit": ((n, 3), torch.float64)}
    t = {k: torch.full(s, 77, dtype=d, device="cuda") for k, (s, d) in shapes.items() if k not in skip}
    nd = None if normals is None else torch.from_numpy(np.array(normals, dtype=np.float64)).cuda()   # (a copy: the shared references are read-only)
    ptr = {k: (t[k].data_ptr() if k in t else 0) for k in OUTPUTS}
    nsig = alg.m3c2_device(core, ref, cmp, radius, depth, 0 if nd is None else nd.data_ptr(), min_points, reg, orient, ptr["distance"], ptr["lod"], ptr["significant"],
                           ptr["counts"], ptr["sums"], ptr["unit"], count_significant="n_significant" not in skip)
    out = {k: v.cpu().numpy() for k, v in t.items()}
    if "counts" in out:
        out["counts"] = out["counts"].view(np.uint32)
    out["n_significant"] = nsig
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "n_significant":
            assert a[k] == b[k]
        else:
            assert a[k].tobytes() == b[k].tobytes(), f"{k} differs between two calls"


def run(hip, core_pts, ref, cmp, radius, depth, normals=None, min_points=4, reg=0.0, orient=False, storage="H", skip=()):
    """The device's outputs as numpy arrays; computed twice, and the two calls agree in every bit"""
    core = core_pts if hasattr(core_pts, "_h") else core_buffer(hip, core_pts, storage)
    a = run_once(core, ref, cmp, radius, depth, normals, min_points, reg, orient, skip)
    b = run_once(core, ref, cmp, radius, depth, normals, min_points, reg, orient, skip)
    same_bits(a, b)
    return a


def check(dev, want, min_points=4, reg=0.0, what=""):
    """The assertions of every case (module docstring)"""
    n = len(want["counts"])
    if "unit" in dev:
        bad = np.flatnonzero((bits(dev["unit"]) != bits(want["u"])).any(axis=1))
        assert bad.size == 0, f"{what}: unit normals differ at {bad[:4]}: {dev['unit'][bad[:4]]} vs {want['u'][bad[:4]]}"
    if "counts" in dev:
        bad = np.flatnonzero((dev["counts"] != want["counts"]).any(axis=1))
        assert bad.size == 0, f"{what}: counts differ at {bad[:4]}: {dev['counts'][bad[:4]]} vs {want['counts'][bad[:4]]}"
    if "sums" in dev:
        m = np.repeat(want["counts"].astype(np.float64), 2, axis=1)
        bound = 2.0 * m * EPS * want["abs"]
        err = np.abs(dev["sums"] - want["sums"])
        bad = np.flatnonzero((~(err <= bound)).any(axis=1))
        assert bad.size == 0, f"{what}: sums beyond the bound at {bad[:4]}: {err[bad[:4]]} vs {bound[bad[:4]]}"
    if "counts" in dev and "sums" in dev:
        valid = want["valid"] if "unit" not in dev else ~np.isnan(dev["unit"][:, 0])
        d, l, s = M.finish(dev["counts"], dev["sums"], valid, min_points, reg)
        if "distance" in dev:
            assert np.array_equal(bits(dev["distance"]), bits(d)), f"{what}: distance is not the formula on the device's own sums"
        if "lod" in dev:
            assert np.array_equal(bits(dev["lod"]), bits(l)), f"{what}: lod is not the formula on the device's own sums"
        if "significant" in dev:
            assert np.array_equal(dev["significant"], s.astype(np.uint8)), f"{what}: significance is not the formula on the device's own sums"
    if "significant" in dev:
        assert set(np.unique(dev["significant"])) <= {0, 1}
        if dev["n_significant"] is not None:
            assert dev["n_significant"] == int(dev["significant"].sum()), what
    for k in dev:
        if k != "n_significant":
            assert len(dev[k]) == n


def rng_cloud(seed, n, lo=-4.0, hi=4.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def random_units(seed, n):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v * np.random.default_rng(seed + 1).uniform(0.5, 3.0, (n, 1))     # (not of unit length: the kernel normalises)


# ------------------------------------------------------------------------------------------------------------------------ GPU: core-point count

def _count_case():
    core = rng_cloud(1, 4 * LANES + 1, -3.5, 3.5)
    c1, c2 = rng_cloud(2, 3001), rng_cloud(3, 2999) + [0.0, 0.0, 0.05]
    normals = random_units(4, len(core))
    return core, c1, c2, normals, M.m3c2(core, c1, c2, 0.9, 2.5, normals=normals)


CORE_COUNTS = [1, CORES - 1, CORES, CORES + 1, 2 * CORES - 1, 2 * CORES, 2 * CORES + 1, 4 * LANES - 1, 4 * LANES, 4 * LANES + 1]


@pytest.mark.gpu
def test_kernel_shape_on_the_gpu(hip):
    assert alg.m3c2_kernel_shape(hip) == {"cores_per_block": CORES, "lanes_per_core": LANES}


@pytest.mark.gpu
def test_core_point_counts(hip):
    """Every seam of cores_per_block, one core point, and an empty core buffer"""
    core, c1, c2, normals, want = reference("m3c2-count", _count_case)
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        for k in CORE_COUNTS:
            dev = run(hip, core[:k], ref, cmp, 0.9, 2.5, normals[:k])
            check(dev, {key: v[:k] for key, v in want.items()}, what=f"{k} core points")
        assert want["counts"].min() > 0 and want["significant"].any() and not want["significant"].all()
        empty = _empty_buffer(hip)
        assert alg.m3c2_device(empty, ref, cmp, 0.9, 2.5, normals_ptr=8, distance_ptr=8) == 0
    finally:
        ref.destroy()
        cmp.destroy()


# ---------------------------------------------------------------------------------------------------------------------------- GPU: member count

MEMBER_COUNTS = [0, 1, 15, 16, 17, LANES - 1, LANES, LANES + 1, 2 * LANES + 1, 5000]


def _axis_cloud(m, seed):
    """m points on the z axis within |z| <= 1, so exactly m members for a core point at the origin with a vertical normal, R = 0.5, L = 1; points
    beyond the caps and beside the cylinder, and two far corners that make the cell large"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1.0, 1.0, m)
    if m >= 2:
        z[0], z[1] = 1.0, -1.0                                  # on the caps: inclusive
    on_axis = np.column_stack([np.zeros(m), np.zeros(m), z])
    beyond = np.array([[0.0, 0.0, 1.0 + 2.0 ** -40], [0.0, 0.0, -1.5], [0.5 + 2.0 ** -40, 0.0, 0.0], [0.4, 0.4, 0.0], [-30.0, -30.0, -30.0], [30.0, 30.0, 30.0]])
    return np.concatenate([beyond[:3], on_axis, beyond[3:]])


@pytest.mark.gpu
@pytest.mark.parametrize("m", MEMBER_COUNTS)
def test_member_counts(hip, m):
    """Exact by construction; 5 000 members share ONE cell (an edge of 10 around the axis)"""
    c1, c2 = _axis_cloud(m, 10 + m), _axis_cloud(max(m, 4), 20 + m) + [0.0, 0.0, 0.0]
    core = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0]])
    want = reference(("m3c2-members", m), lambda: M.m3c2(core, c1, c2, 0.5, 1.0, normals=np.tile(UP, (2, 1)), min_points=1))
    assert want["counts"][0, 0] == m and want["counts"][1].sum() == 0
    ref, cmp = index_of(hip, c1, 10.0), index_of(hip, c2, 10.0 if m == 5000 else 0.0)
    try:
        if m == 5000:
            g = ref.grid()
            assert g["cell_edge"] == 10.0
        check(run(hip, core, ref, cmp, 0.5, 1.0, np.tile(UP, (2, 1)), min_points=1), want, min_points=1, what=f"{m} members")
    finally:
        ref.destroy()
        cmp.destroy()


# ----------------------------------------------------------------------------------------------------------------------------- GPU: knife edges

def _knife_cloud(R, L, seed):
    """Points exactly on and one ulp beyond the caps and the side of the cylinder (origin, vertical normal), background points, and the corners
    (-8, -8, -8) and (8, 8, 8): with a power-of-two edge every cell boundary is a binary fraction, and the caps z = +-L and the side
    x, y = +-R lie exactly on boundaries."""
    up = lambda v: np.nextafter(v, INF)
    special = []
    inside = []
    for sign in (1.0, -1.0):
        special += [[0.0, 0.0, sign * L], [0.0, 0.0, sign * up(L)], [sign * R, 0.0, 0.0], [sign * up(R), 0.0, 0.0], [0.0, sign * R, 0.0], [0.0, sign * up(R), 0.0],
                    [sign * R, 0.0, sign * L], [sign * R, 0.0, sign * up(L)], [0.0, sign * up(R), -sign * L]]
        inside += [True, False, True, False, True, False, True, False, False]
    background = rng_cloud(seed, 400, -8.0, 8.0)
    return np.concatenate([np.array(special), background, [[-8.0, -8.0, -8.0], [8.0, 8.0, 8.0]]]), np.array(inside)


@pytest.mark.gpu
def test_knife_edges(hip):
    """t == L is in and nextafter(L) is out, the same for -L; a perpendicular distance of exactly R is in and one ulp beyond is out.  With the
    automatic edge times 0.3, 1 and 5 on either index the special points fall into the core point's cell or a neighbouring one; with edges of
    0.25, 1 and 4 the caps and the side lie exactly on cell boundaries."""
    core = np.array([[0.0, 0.0, 0.0]])
    for R, L in ((1.0, 2.0), (4.0, 4.0), (0.75, 1.25)):
        (c1, in1), (c2, in2) = _knife_cloud(R, L, 31), _knife_cloud(R, L, 32)
        want = reference(("m3c2-knife", R, L), lambda: M.m3c2(core, c1, c2, R, L, normals=[UP], min_points=1))
        t1 = M.member_terms(core[0], UP, c1[:len(in1)], R, L)
        assert len(t1) == in1.sum() == 8                        # the hand-made answers: exactly the points marked inside
        a1, a2 = auto_edge(hip, c1), auto_edge(hip, c2)
        edges = [(f1 * a1, f2 * a2) for f1, f2 in itertools.product((0.3, 1.0, 5.0), repeat=2)] + list(itertools.product((0.25, 1.0, 4.0), repeat=2))
        for e1, e2 in edges:
            ref, cmp = index_of(hip, c1, e1), index_of(hip, c2, e2)
            try:
                check(run(hip, core, ref, cmp, R, L, [UP], min_points=1), want, min_points=1, what=f"R {R} L {L} edges {e1} {e2}")
            finally:
                ref.destroy()
                cmp.destroy()


# ----------------------------------------------------------------------------------------------------------------------- GPU: grid independence

def _grid_case():
    core = rng_cloud(41, 301, -3.0, 3.0)
    c1, c2 = rng_cloud(42, 5003), rng_cloud(43, 4999)
    normals = random_units(44, len(core))
    return core, c1, c2, normals, M.m3c2(core, c1, c2, 0.7, 1.9, normals=normals)


@pytest.mark.gpu
def test_grid_independence(hip):
    """The same clouds indexed at 0.3, 1 and 5 times the automatic edge: counts identical, sums within the bound"""
    core, c1, c2, normals, want = reference("m3c2-grid", _grid_case)
    a1, a2 = auto_edge(hip, c1), auto_edge(hip, c2)
    seen = []
    for f1, f2 in itertools.product((0.3, 1.0, 5.0), repeat=2):
        ref, cmp = index_of(hip, c1, f1 * a1), index_of(hip, c2, f2 * a2)
        try:
            dev = run(hip, core, ref, cmp, 0.7, 1.9, normals)
            check(dev, want, what=f"edges x{f1} x{f2}")
            seen.append(dev["counts"])
        finally:
            ref.destroy()
            cmp.destroy()
    assert all(np.array_equal(seen[0], s) for s in seen[1:])


# ---------------------------------------------------------------------------------------------------------------------------------- GPU: normals

STENCIL = np.array([d for d in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(d)])


def _normals_case():
    """The 26 directions of the stencil and random ones, L = 40 R: core points in the middle, next to each of the six faces, and at the eight
    corners, so that the cylinders leave the grid on every side"""
    spots = np.array([[0.0, 0.0, 0.0], [3.9, 0.0, 0.0], [-3.9, 0.0, 0.0], [0.0, 3.9, 0.0], [0.0, -3.9, 0.0], [0.0, 0.0, 3.9], [0.0, 0.0, -3.9], [3.9, 3.9, 3.9], [-3.9, -3.9, -3.9]])
    dirs = np.concatenate([STENCIL, random_units(51, 14)])
    core = np.repeat(spots, len(dirs), axis=0)
    normals = np.tile(dirs, (len(spots), 1))
    c1, c2 = rng_cloud(52, 6001), rng_cloud(53, 5999) + [0.02, -0.01, 0.03]
    return core, c1, c2, normals, M.m3c2(core, c1, c2, 0.25, 10.0, normals=normals)


@pytest.mark.gpu
def test_normals_and_cylinders_that_leave_the_grid(hip):
    core, c1, c2, normals, want = reference("m3c2-normals", _normals_case)
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        check(run(hip, core, ref, cmp, 0.25, 10.0, normals), want, what="L = 40 R")
        assert want["counts"].max() > 20 and (want["counts"] == 0).any()      # (cylinders that point out of a corner hold little or nothing)
        # a cylinder larger than both clouds: out on all sides, every finite point a member
        big = M.m3c2(core[:3], c1, c2, 20.0, 20.0, normals=normals[:3])
        assert np.array_equal(big["counts"], [[6001, 5999]] * 3)
        check(run(hip, core[:3], ref, cmp, 20.0, 20.0, normals[:3]), big, what="all sides")
    finally:
        ref.destroy()
        cmp.destroy()


_WORK_SCRIPT = r"""
import numpy as np, torch
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointLayout, attributes as A
hip = pa.product_api()
def buf(p):
    b = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=hip))
    b.resize(len(p)); b.set_attribute_range(A.POSITION_3D, range(0, len(p)), np.ascontiguousarray(p)); return b
rng = np.random.default_rng(5)
c1, c2 = rng.uniform(-4, 4, (4000, 3)), rng.uniform(-4, 4, (4000, 3))
ref, cmp = alg.NearestNeighbourIndex(buf(c1)), alg.NearestNeighbourIndex(buf(c2))
normals = np.tile([0.0, 0.0, 1.0], (64, 1))
far = buf(rng.uniform(-4, 4, (64, 3)) + [500.0, 0.0, 0.0])
r = alg.m3c2(far, ref, cmp, 0.5, 3.0, normals=normals)
print("far", alg.m3c2_work(hip), int(r.counts.sum()))
near = buf(rng.uniform(-3, 3, (64, 3)))
r = alg.m3c2(near, ref, cmp, 0.5, 3.0, normals=normals)
w = alg.m3c2_work(hip)
print("near", w["members"] == int(r.counts.sum()), w["candidates"] >= w["members"] > 0, w["rows"] > 0, w["candidates"] < 64 * 8000)
print("times", all(t > 0.0 for t in alg.m3c2_phase_times(hip)[1:]))
"""


@pytest.mark.gpu
def test_work_counters_and_phase_times(hip):
    """Core points far outside both clouds cost no search: zero rows, zero candidates.  The switches are read once per process, hence the child;
    in THIS process, without them, both report zeros."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PST_M3C2_WORK="1", PST_M3C2_TIMES="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _WORK_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "far {'rows': 0, 'candidates': 0, 'members': 0} 0" in r.stdout, r.stdout
    assert "near True True True True" in r.stdout and "times True" in r.stdout, r.stdout
    if not os.environ.get("PST_M3C2_WORK"):
        assert alg.m3c2_work(hip) == {"rows": 0, "candidates": 0, "members": 0}


# ---------------------------------------------------------------------------------------------------------------------- GPU: invalid core points

@pytest.mark.gpu
def test_invalid_core_points_and_points_that_are_not_finite(hip):
    """NaN and inf in core points; NaN, inf, zero and underflowing normals; points that are not finite inside both clouds are never members"""
    c1, c2 = rng_cloud(61, 2000), rng_cloud(62, 2000)
    c1[::50, 0], c1[7::50, 2], c2[::40, 1], c2[3::40, 0] = NAN, INF, -INF, NAN
    core = rng_cloud(63, 40, -2.0, 2.0)
    normals = random_units(64, 40)
    core[1, 0], core[2, 1], core[3, 2], core[4] = NAN, INF, -INF, NAN
    normals[10, 0], normals[11, 1], normals[12, 2], normals[13], normals[14] = NAN, INF, -INF, 0.0, [1e-170, -1e-170, 1e-170]
    normals[15], normals[16] = [1e200, 1e200, 0.0], [0.0, -0.0, 5e-324]          # nn overflows; nn underflows to 0
    normals[17] = [1e-150, 0.0, 0.0]                                              # nn is subnormal but not 0: valid
    want = M.m3c2(core, c1, c2, 1.0, 2.0, normals=normals, min_points=2)
    assert list(np.flatnonzero(~want["valid"])) == [1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 16] and want["valid"][17]
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        dev = run(hip, core, ref, cmp, 1.0, 2.0, normals, min_points=2)
        check(dev, want, min_points=2, what="invalid")
        bad = ~want["valid"]
        assert not dev["counts"][bad].any() and not dev["sums"][bad].any() and np.isnan(dev["distance"][bad]).all() and not dev["significant"][bad].any()
    finally:
        ref.destroy()
        cmp.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["reference", "compared", "both"])
def test_index_without_a_finite_point(hip, which):
    blank = np.full((5, 3), NAN)
    c1 = blank if which in ("reference", "both") else rng_cloud(65, 500)
    c2 = blank if which in ("compared", "both") else rng_cloud(66, 500)
    core, normals = rng_cloud(67, 9, -2.0, 2.0), random_units(68, 9)
    want = M.m3c2(core, c1, c2, 1.5, 2.0, normals=normals, min_points=1)
    ref, cmp = index_of(hip, c1, normals=np.tile(UP, (5, 1)) if which != "compared" else None), index_of(hip, c2)
    try:
        dev = run(hip, core, ref, cmp, 1.5, 2.0, normals, min_points=1)
        check(dev, want, min_points=1, what=which)
        assert np.isnan(dev["distance"]).all() and dev["n_significant"] == 0
        if which != "compared":       # nearest-normal mode on a reference without a finite point: no nearest point, every core point invalid
            near = run(hip, core, ref, cmp, 1.5, 2.0, None, min_points=1)
            check(near, M.m3c2(core, c1, c2, 1.5, 2.0, reference_normals=np.tile(UP, (5, 1)), min_points=1), min_points=1)
            assert np.isnan(near["unit"]).all() and not near["counts"].any()
    finally:
        ref.destroy()
        cmp.destroy()


# ------------------------------------------------------------------------------------------------------------------------------ GPU: min_points

@pytest.mark.gpu
def test_min_points(hip):
    """min_points 1, 2 and 4 against 0 .. 4 members on either side: 25 core points along x, each with its own little column of points"""
    pairs = list(itertools.product(range(5), repeat=2))
    core = np.array([[10.0 * k, 0.0, 0.0] for k in range(len(pairs))])
    rng = np.random.default_rng(71)
    c1 = np.array([c + [0.0, 0.0, z] for c, (a, b) in zip(core, pairs) for z in rng.uniform(-0.5, 0.5, a)] + [[-5.0, 0.0, 0.0]])
    c2 = np.array([c + [0.0, 0.0, z] for c, (a, b) in zip(core, pairs) for z in rng.uniform(0.0, 1.0, b)] + [[-5.0, 0.0, 0.0]])
    normals = np.tile(UP, (len(core), 1))
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        for mp in (1, 2, 4):
            want = M.m3c2(core, c1, c2, 0.5, 1.0, normals=normals, min_points=mp, registration_error=0.01)
            assert np.array_equal(want["counts"], pairs)
            dev = run(hip, core, ref, cmp, 0.5, 1.0, normals, min_points=mp, reg=0.01)
            check(dev, want, min_points=mp, reg=0.01, what=f"min_points {mp}")
            enough = np.array([a >= mp and b >= mp for a, b in pairs])
            spread = np.array([a >= 2 and b >= 2 for a, b in pairs])
            assert np.array_equal(~np.isnan(dev["distance"]), enough) and np.array_equal(~np.isnan(dev["lod"]), enough & spread)
            assert not dev["significant"][~(enough & spread)].any()
    finally:
        ref.destroy()
        cmp.destroy()


# ------------------------------------------------------------------------------------------------------------------------------ GPU: orientation

@pytest.mark.gpu
def test_orient_up(hip):
    """uz negative, zero and positive, with the uy and ux tie-breaks: where the normal is turned over, the distance changes sign exactly"""
    dirs = np.array([[0.3, 0.2, -1.0], [0.3, 0.2, 1.0], [0.5, -1.0, 0.0], [0.5, 1.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, -0.0, -0.0], [0.0, -2.0, 0.0],
                     [0.0, 0.0, -3.0], [-1.0, 1.0, -1e-300]])
    core = rng_cloud(81, len(dirs), -1.0, 1.0)
    c1, c2 = rng_cloud(82, 4000, -3.0, 3.0), rng_cloud(83, 4000, -3.0, 3.0) * [1.0, 1.0, 0.9]
    flipped = np.array([True, False, True, False, True, False, True, True, True, True])
    plain = M.m3c2(core, c1, c2, 0.8, 1.5, normals=dirs)
    up = M.m3c2(core, c1, c2, 0.8, 1.5, normals=dirs, flags=M.ORIENT_UP)
    assert np.array_equal(up["u"], np.where(flipped[:, None], -plain["u"], plain["u"])) and plain["counts"].min() >= 4
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        d_plain, d_up = run(hip, core, ref, cmp, 0.8, 1.5, dirs), run(hip, core, ref, cmp, 0.8, 1.5, dirs, orient=True)
        check(d_plain, plain, what="as given")
        check(d_up, up, what="ORIENT_UP")
        assert np.array_equal(d_up["counts"], d_plain["counts"])
        assert np.array_equal(bits(d_up["distance"]), bits(np.where(flipped, -d_plain["distance"], d_plain["distance"])))
        assert np.array_equal(bits(d_up["lod"]), bits(d_plain["lod"]))
    finally:
        ref.destroy()
        cmp.destroy()


# ------------------------------------------------------------------------------------------------------------------------- GPU: nearest normals

@pytest.mark.gpu
def test_nearest_normal_mode_with_ties(hip):
    """Reference points on a lattice and core points on lattice mid-points: 2, 4 and 8 reference points tie, the lowest buffer index gives the normal"""
    c1 = lattice(9) - 4.0
    order = np.random.default_rng(91).permutation(len(c1))
    c1 = c1[order]
    ref_normals = random_units(92, len(c1))
    c2 = c1 + [0.0, 0.0, 0.125]
    core = np.concatenate([lattice(4) - 1.5 + off for off in ([0.5, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.5, 0.5], [0.25, 0.0, 0.0])] + [[[NAN, 0.0, 0.0]]])
    want = M.m3c2(core, c1, c2, 1.25, 2.0, reference_normals=ref_normals)
    idx, _ = nn_ref.nearest(core, c1)
    picked, _ = M.nearest_normals(core, c1, ref_normals)
    assert np.array_equal(picked[:-1], ref_normals[idx[:-1]]) and not want["valid"][-1] and want["valid"][:-1].all()
    ref, cmp = index_of(hip, c1, normals=ref_normals), index_of(hip, c2)
    try:
        near = run(hip, core, ref, cmp, 1.25, 2.0, None)
        check(near, want, what="nearest normals")
        given = run(hip, core, ref, cmp, 1.25, 2.0, picked)           # the same normals handed over as d_normals: the same bits
        same_bits({k: v for k, v in near.items()}, {k: v for k, v in given.items()})
    finally:
        ref.destroy()
        cmp.destroy()


@pytest.mark.gpu
def test_with_normals_index_agrees_with_its_normals_passed(hip):
    """NearestNeighbourIndex.with_normals: the normals the index holds, read back through d_unit_normals of a run whose core points ARE the
    reference points (each its own nearest point... up to duplicates: none here), give the same bits when passed as d_normals"""
    import torch
    pts = rng_cloud(95, 3000) * [1.0, 1.0, 0.05]
    c2 = pts + [0.0, 0.0, 0.1]
    buf = buffer_of(hip, pts)
    ref, cmp = alg.NearestNeighbourIndex.with_normals(buf, 12), index_of(hip, c2)
    try:
        normals = torch.zeros((len(pts), 3), dtype=torch.float64, device="cuda")
        alg.compute_normals_device(buf, 12, normals_ptr=normals.data_ptr())
        torch.cuda.synchronize()
        core = rng_cloud(96, 500, -3.5, 3.5) * [1.0, 1.0, 0.05]
        near = run(hip, core, ref, cmp, 0.6, 1.0, None)
        check(near, M.m3c2(core, pts, c2, 0.6, 1.0, reference_normals=normals.cpu().numpy()), what="with_normals")
        own = run(hip, pts, ref, cmp, 0.6, 1.0, None)
        same_bits(own, run(hip, pts, ref, cmp, 0.6, 1.0, normals.cpu().numpy()))
        # the Python wrapper on buffers builds the same index itself
        r = alg.m3c2(core_buffer(hip, core), buf, buffer_of(hip, c2), 0.6, 1.0, k_nn=12, return_sums=True)
        assert np.array_equal(bits(r.distance), bits(near["distance"])) and np.array_equal(r.counts, near["counts"]) and r.n_significant == near["n_significant"]
        assert np.array_equal(bits(r.unit_normals), bits(near["unit"])) and np.array_equal(r.significant, near["significant"].astype(bool))
        with np.errstate(all="ignore"):
            q = r.sums[:, 1] - r.sums[:, 0] * r.sums[:, 0] / r.counts[:, 0]
            spread = np.sqrt(np.where(q > 0, q, 0.0) / (r.counts[:, 0].astype(np.int64) - 1))
        ok = r.counts[:, 0] >= 2
        assert np.array_equal(bits(r.spread[ok, 0]), bits(spread[ok])) and np.isnan(r.spread[~ok, 0]).all()
    finally:
        ref.destroy()
        cmp.destroy()


# --------------------------------------------------------------------------------------------------------------------------------- GPU: storages

@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["V", "H", "packedV", "external", "sliceV", "sliceH"])
def test_core_buffer_storages(hip, storage):
    core, c1, c2, normals, want = reference("m3c2-count", _count_case)
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    try:
        check(run(hip, core[:101], ref, cmp, 0.9, 2.5, normals[:101], storage=storage), {k: v[:101] for k, v in want.items()}, what=storage)
    finally:
        ref.destroy()
        cmp.destroy()


@pytest.mark.gpu
def test_every_output_is_optional(hip):
    core, c1, c2, normals, want = reference("m3c2-count", _count_case)
    ref, cmp = index_of(hip, c1), index_of(hip, c2)
    part = {k: v[:33] for k, v in want.items()}
    try:
        full = run(hip, core[:33], ref, cmp, 0.9, 2.5, normals[:33])
        for left_out in OUTPUTS + ("n_significant",):
            dev = run(hip, core[:33], ref, cmp, 0.9, 2.5, normals[:33], skip=(left_out,))
            check(dev, part, what=f"without {left_out}")
            for k in dev:
                if k != "n_significant":
                    assert dev[k].tobytes() == full[k].tobytes()
        only = run(hip, core[:33], ref, cmp, 0.9, 2.5, normals[:33], skip=OUTPUTS)
        assert only["n_significant"] == full["n_significant"]
    finally:
        ref.destroy()
        cmp.destroy()


# ------------------------------------------------------------------------------------------------------------------------------- GPU: realistic

REG = 0.03               # 1.96 * (0.0023 + 0.03) = 0.063 lies above the planes' offset of 0.05 and far below the patch's 0.55


def noisy_planes(seed=101, n=20003, n_core=2003):
    """Two noisy planes 0.05 apart (sigma 0.01), a patch of the second raised by 0.5; core points thinned from the first"""
    rng = np.random.default_rng(seed)
    p1 = np.column_stack([rng.uniform(0.0, 20.0, (n, 2)), rng.normal(0.0, 0.01, n)])
    p2 = np.column_stack([rng.uniform(0.0, 20.0, (n, 2)), 0.05 + rng.normal(0.0, 0.01, n)])
    patch = (np.abs(p2[:, 0] - 12.0) < 2.0) & (np.abs(p2[:, 1] - 7.0) < 1.5)
    p2[patch, 2] += 0.5
    core = p1[rng.choice(n, n_core, replace=False)]
    return p1, p2, core


def _realistic_case():
    p1, p2, core = noisy_planes()
    normals = np.tile(UP, (len(core), 1))
    return p1, p2, core, normals, M.m3c2(core, p1, p2, 0.5, 1.0, normals=normals, registration_error=REG)


def margin_of(want, reg):
    """|distance| - lod and the bound on what ANY summation order of the four sums can move it: the propagated worst case (first order, with a
    factor 4 to spare), used only to show that no core point of the case sits on the fence"""
    c, s, a = want["counts"].astype(np.float64), want["sums"], want["abs"]
    ds = 2.0 * np.repeat(c, 2, axis=1) * EPS * a                                  # per sum
    with np.errstate(all="ignore"):
        d_dist = ds[:, 0] / c[:, 0] + ds[:, 2] / c[:, 1]
        var = [np.maximum(s[:, 2 * x + 1] - s[:, 2 * x] ** 2 / c[:, x], 0.0) / (c[:, x] - 1) for x in (0, 1)]
        d_var = [(ds[:, 2 * x + 1] + 2.0 * np.abs(s[:, 2 * x]) * ds[:, 2 * x] / c[:, x]) / (c[:, x] - 1) for x in (0, 1)]
        root = np.sqrt(var[0] / c[:, 0] + var[1] / c[:, 1])
        d_lod = 1.96 * (d_var[0] / c[:, 0] + d_var[1] / c[:, 1]) / (2.0 * root)
        return np.abs(want["distance"]) - want["lod"], 4.0 * (d_dist + d_lod) + 16.0 * EPS * (np.abs(want["distance"]) + want["lod"])


def test_realistic_case_has_no_core_point_on_the_fence():
    """CPU: with naive np.sum against fsum no core point's |distance| - lod lies within the propagated sum bound, so the device's mask must EQUAL
    the restatement's (the GPU test below asserts it)."""
    p1, p2, core, normals, want = reference("m3c2-real", _realistic_case)
    gap, bound = margin_of(want, REG)
    ok = ~np.isnan(want["distance"])
    assert ok.sum() > 1900 and (np.abs(gap[ok]) > bound[ok]).all() and np.abs(gap[ok]).min() > 1e-6
    assert 40 < want["significant"].sum() < 400                                   # the raised patch, and little else
    inside = (np.abs(core[:, 0] - 12.0) < 1.4) & (np.abs(core[:, 1] - 7.0) < 0.9)
    assert want["significant"][inside].all() and (want["distance"][inside] > 0.5).all()
    # naive summation in cloud order decides every core point like fsum does
    for i in np.flatnonzero(ok)[::40]:
        t1, t2 = M.member_terms(core[i], UP, p1, 0.5, 1.0), M.member_terms(core[i], UP, p2, 0.5, 1.0)
        naive = np.array([[np.sum(t1), np.sum(t1 * t1), np.sum(t2), np.sum(t2 * t2)]])
        _, _, s = M.finish(want["counts"][i:i + 1], naive, [True], 4, REG)
        assert s[0] == want["significant"][i]


@pytest.mark.gpu
def test_realistic_planes_with_a_raised_patch(hip):
    p1, p2, core, normals, want = reference("m3c2-real", _realistic_case)
    ref, cmp = index_of(hip, p1), index_of(hip, p2)
    try:
        dev = run(hip, core, ref, cmp, 0.5, 1.0, normals, reg=REG)
        check(dev, want, reg=REG, what="realistic")
        assert np.array_equal(dev["significant"].astype(bool), want["significant"])
    finally:
        ref.destroy()
        cmp.destroy()
