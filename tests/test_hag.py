"""Height above ground from the k nearest ground points in the XY plane (pst_height_above_ground_device, pst_buffer_u8_equals_mask_device):
the numpy restatement tests/hag_ref.py on hand-computed cases, every check the host answers without a device, and on the GPU the results against
the restatement BIT FOR BIT (NaN where it has NaN): no tolerance appears anywhere."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import hag_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

Q = 64            # asserted against pst_hag_kernel_shape below: the parametrisations need them at collection time
MAX_K = 32
BOUNDS_POINTS = 4096
MASK_POINTS = 1024  # points per workgroup of the equals-mask kernel (pst_pmf_kernel_shape's points_per_block)
STORAGES = ["H", "V", "packedH", "packedV", "external", "sliceH", "sliceV"]
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: {int((~np.isnan(got[nan])).sum())} values should be NaN"
    bad = np.flatnonzero(~nan & (bits(got) != bits(want)))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} differ, first {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"


# ------------------------------------------------------------------------------------------------------------ the restatement, by hand

def test_restatement_on_hand_computed_cases():
    ground = np.array([[0.0, 0.0, 10.0], [1.0, 0.0, 20.0], [0.0, 2.0, 30.0], [5.0, 5.0, 40.0]])
    # k = 1: z - z_nearest
    hag, zg, ng, unres = R.height_above_ground([[0.9, 0.1, 25.0], [4.0, 4.0, 1.0]], ground, k=1)
    assert zg.tolist() == [20.0, 40.0] and hag.tolist() == [5.0, -39.0] and ng == 4 and unres == 0
    # an exact hit ignores the other neighbours
    hag, zg, _, _ = R.height_above_ground([[1.0, 0.0, 21.5]], ground, k=3)
    assert zg.tolist() == [20.0] and hag.tolist() == [1.5]
    # two ground points at distances 1 and 2, k = 2: zg = (z0 + 0.25 * z1) / 1.25
    two = np.array([[1.0, 0.0, 8.0], [0.0, 2.0, 3.0], [100.0, 0.0, 1000.0]])
    hag, zg, _, _ = R.height_above_ground([[0.0, 0.0, 9.0]], two, k=2)
    assert zg[0] == (8.0 + 0.25 * 3.0) / 1.25 and hag[0] == 9.0 - zg[0]
    # fewer than k in reach: those there are; none: NaN and unresolved
    hag, zg, _, unres = R.height_above_ground([[0.0, 0.0, 9.0]], two, k=3, max_distance=2.0)
    assert zg[0] == (8.0 + 0.25 * 3.0) / 1.25 and unres == 0
    hag, zg, _, unres = R.height_above_ground([[0.0, 0.0, 9.0]], two, k=3, max_distance=0.5)
    assert np.isnan(zg[0]) and np.isnan(hag[0]) and unres == 1
    # equal d2 goes to the lower index, whatever the order in the array
    tie = np.array([[0.0, 1.0, 7.0], [1.0, 0.0, 5.0], [-1.0, 0.0, 6.0]])
    assert R.height_above_ground([[0.0, 0.0, 0.0]], tie, k=1)[1][0] == 7.0
    assert R.height_above_ground([[0.0, 0.0, 0.0]], tie[::-1], k=1)[1][0] == 6.0
    assert R.height_above_ground([[0.0, 0.0, 0.0]], tie, k=2)[1][0] == (7.0 + 5.0) / 2.0
    # the mask and non-finite ground points; a query that is not finite is not counted as unresolved
    masked = R.height_above_ground([[0.9, 0.1, 25.0], [np.nan, 0.0, 1.0]], ground, mask=[1, 0, 1, 1], k=1)
    assert masked[1][0] == 10.0 and np.isnan(masked[0][1]) and masked[2] == 3 and masked[3] == 0
    holed = ground.copy()
    holed[1, 2] = np.inf
    assert R.height_above_ground([[0.9, 0.1, 25.0]], holed, k=1)[1][0] == 10.0
    # z takes no part in the distance
    assert R.height_above_ground([[0.1, 0.0, 1e6]], ground, k=1)[1][0] == 10.0


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer, extra=()):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype), *extra], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def test_kernel_shape(hip):
    assert alg.hag_kernel_shape(hip) == {"queries_per_block": Q, "max_k": MAX_K, "bounds_points_per_block": BOUNDS_POINTS}
    assert alg.pmf_kernel_shape(hip)["points_per_block"] == MASK_POINTS
    one = C.c_uint32()
    hip.hag_kernel_shape(None, C.byref(one), None)  # each pointer is optional
    assert one.value == MAX_K
    hip.hag_kernel_shape(None, None, None)
    assert alg.hag_phase_times(hip) == (0.0, 0.0, 0.0)
    assert _code(lambda: hip.hag_phase_times(None)) == 1


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    ng, nu, me, dim = C.c_uint64(7), C.c_uint64(7), (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 2)(1, 1)

    def call(query=buf._h, ground=buf._h, k=3, md=INF, edge=0.0, hag=fake, gz=fake):
        return hip.height_above_ground_device(query, ground, None, k, md, edge, hag, gz, C.byref(ng), C.byref(nu), me, dim)
    assert _code(lambda: call(query=None)) == 1
    assert _code(lambda: call(ground=None)) == 1
    assert _code(lambda: call(hag=None, gz=None)) == 1                          # not both
    assert _code(lambda: call(k=0)) == 1
    assert _code(lambda: call(k=MAX_K + 1)) == 1
    for md in (0.0, -1.0, float("nan"), -INF, 1e-200, 1e-155):                  # (the squares of the last two are 0 and subnormal)
        assert _code(lambda: call(md=md)) == 1
    for edge in (-1.0, float("nan"), INF, -INF):
        assert _code(lambda: call(edge=edge)) == 1
    # a position that is not Vec3f64 is known from the layout alone, in either buffer
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: call(query=f32._h)) == 4
    assert _code(lambda: call(ground=f32._h)) == 4
    with pytest.raises(PasturePanic):
        call(ground=f32._h)
    # the parameters come before the layout
    assert _code(lambda: call(query=f32._h, k=0)) == 1
    # an empty query: PST_OK on the host, nothing written, zeros in the counts and the grid; either output alone, and every optional pointer absent
    assert call() == 0 and call(hag=None) == 0 and call(gz=None) == 0
    assert (ng.value, nu.value, list(me), list(dim)) == (0, 0, [0.0, 0.0, 0.0], [0, 0])
    assert hip.height_above_ground_device(buf._h, buf._h, None, MAX_K, 1e-150, 5.0, fake, None, None, None, None, None) == 0
    # the mask call: null arguments, an attribute the layout does not have, one that is not U8; an empty buffer is answered on the host
    cls = _empty_buffer(hip, extra=[A.CLASSIFICATION, A.INTENSITY])
    assert _code(lambda: hip.buffer_u8_equals_mask_device(None, b"Classification", 2, fake)) == 1
    assert _code(lambda: hip.buffer_u8_equals_mask_device(cls._h, None, 2, fake)) == 1
    assert _code(lambda: hip.buffer_u8_equals_mask_device(buf._h, b"Classification", 2, fake)) == 4
    assert _code(lambda: hip.buffer_u8_equals_mask_device(cls._h, b"Intensity", 2, fake)) == 4
    assert hip.buffer_u8_equals_mask_device(cls._h, b"Classification", 2, None) == 0
    alg.classification_mask(cls, 2, 0)


_NO_DEVICE_SCRIPT = r"""
import ctypes as C
import numpy as np
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.buffers import ExternalMemoryBuffer
from pasture_amd.layout import PointLayout, attributes as A
hip = pa.product_api()
points = np.arange(30.0).reshape(10, 3)  # ten points in host memory
buf = ExternalMemoryBuffer(points.ctypes.data, PointLayout.from_attributes([A.POSITION_3D], api=hip), nbytes=points.nbytes)
classes = np.full(10, 2, dtype=np.uint8)
cls = ExternalMemoryBuffer(classes.ctypes.data, PointLayout.from_attributes([A.CLASSIFICATION], api=hip), nbytes=classes.nbytes)
assert buf.len() == 10 and cls.len() == 10
calls = [lambda: alg.height_above_ground_device(buf, None, 3, hag_ptr=8), lambda: alg.height_above_ground_device(buf, 8, 1, 2.0, buf, 0.5, 0, 8),
         lambda: alg.classification_mask(cls, 2, 8)]
out = []
for call in calls:
    try:
        call()
        out.append((0, ""))
    except pa.PastureError as e:
        out.append((e.code, "no CPU fallback" in str(e)))
print("codes", out)
"""


def test_no_cpu_fallback_without_device(hip):
    """Without a GPU the compute calls on NON-EMPTY buffers are PST_ERR_NO_DEVICE, never a CPU path.  An owned buffer cannot hold a point without a
    device, but caller's host memory can be wrapped as one when the library is told not to ask the runtime about the range
    (PST_EXTERNAL_UNCHECKED, read once per process: hence the child process)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PST_EXTERNAL_UNCHECKED="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"codes {[(21, True)] * 3}" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

def device_bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def gpu_hag(hip, query, ground=None, mask=None, k=1, md=INF, edge=0.0, want="both", sq="H", sg="H", bufs=None):
    """(hag or None, ground_z or None, info) through the C entry point; ground None: the query buffer itself.  bufs: (query, ground) buffers made before"""
    import torch
    if bufs is None:
        qb = make_buffer(hip, query, sq)
        gb = qb if ground is None else make_buffer(hip, ground, sg)
    else:
        qb, gb = bufs
    nq = qb.len()
    m = device_bytes(mask) if mask is not None else None
    hag = torch.full((max(nq, 1),), -7.0, dtype=torch.float64, device="cuda") if want in ("both", "hag") else None
    gz = torch.full((max(nq, 1),), -7.0, dtype=torch.float64, device="cuda") if want in ("both", "gz") else None
    info = alg.height_above_ground_device(qb, m.data_ptr() if m is not None and m.numel() else None, k, md, gb, edge, hag.data_ptr() if hag is not None else 0,
                                          gz.data_ptr() if gz is not None else 0)
    torch.cuda.synchronize()
    return (hag.cpu().numpy()[:nq] if hag is not None else None, gz.cpu().numpy()[:nq] if gz is not None else None, info)


def check(hip, query, ground=None, mask=None, k=1, md=INF, edge=0.0, what="", **kw):
    """run the device and compare everything with the restatement; returns the device's info"""
    hag, gz, info = gpu_hag(hip, query, ground, mask, k, md, edge, **kw)
    want = R.height_above_ground(query, query if ground is None else ground, mask, k, md)
    assert_same_bits(hag, want[0], f"{what} hag")
    assert_same_bits(gz, want[1], f"{what} ground_z")
    assert (info["n_ground"], info["n_unresolved"]) == (want[2], want[3]), f"{what}: counts {info} vs {want[2:]}"
    return info


def terrain(n, seed, extent=100.0):
    """n points on rolling ground: x, y uniform in [0, extent)^2"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * extent
    return np.column_stack([xy, 0.02 * xy[:, 0] + 1.5 * np.sin(xy[:, 0] / 15.0) * np.cos(xy[:, 1] / 18.0) + rng.normal(0.0, 0.02, n)])


def queries(n, seed, extent=100.0, margin=10.0):
    """n points over the same square and a margin around it (the clamp), well above the ground"""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.random((n, 2)) * (extent + 2 * margin) - margin, rng.random(n) * 30.0])


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 2, Q - 1, Q, Q + 1, 3 * Q + 5])
def test_query_counts_around_the_seams(hip, nq):
    ground = terrain(500, 1)
    for k, md in ((1, INF), (3, INF), (10, 12.0)):
        check(hip, queries(nq, 2 + nq), ground, k=k, md=md, what=f"nq {nq} k {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [1, 3, 4, 5, BOUNDS_POINTS - 1, BOUNDS_POINTS, BOUNDS_POINTS + 1, 2 * BOUNDS_POINTS + 3])
def test_ground_counts_around_the_seams(hip, ng):
    """k = 4: fewer, as many and more ground points than k; one, exactly one and more than one block partial of the bounds, with and without a mask"""
    ground, q = terrain(ng, 3), queries(70, 4)
    check(hip, q, ground, k=4, what=f"ng {ng}")
    mask = (np.arange(ng) % 3 != 1).astype(np.uint8)
    mask[-1] = 1  # (the last block's only point of G when ng = BOUNDS_POINTS + 1)
    check(hip, q, ground, mask=mask, k=4, md=30.0, what=f"ng {ng} masked")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 10, 16, MAX_K])
def test_every_k(hip, k):
    ground, q = terrain(700, 5), queries(300, 6)
    check(hip, q, ground, k=k, what=f"k {k}")
    check(hip, q, ground, k=k, md=9.0, what=f"k {k} bounded")


@pytest.mark.gpu
@pytest.mark.parametrize("sg", STORAGES)
@pytest.mark.parametrize("sq", STORAGES)
def test_storages(hip, sq, sg):
    ground, q = terrain(300, 7), queries(130, 8)
    mask = (np.arange(300) % 5 != 0).astype(np.uint8)
    check(hip, q, ground, mask=mask, k=5, sq=sq, sg=sg, what=f"{sq} / {sg}")


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "packedV"])
def test_query_is_ground_and_two_buffers(hip, storage):
    pts = np.concatenate([terrain(400, 9), queries(200, 10, margin=0.0)])
    is_ground = (np.arange(600) < 400).astype(np.uint8)
    rng = np.random.default_rng(11)
    order = rng.permutation(600)
    pts, is_ground = pts[order], is_ground[order]
    hag, gz, info = gpu_hag(hip, pts, None, is_ground, k=3, sq=storage)
    want = R.height_above_ground(pts, pts, is_ground, 3)
    assert_same_bits(hag, want[0], "same buffer hag")
    assert_same_bits(gz, want[1], "same buffer ground_z")
    assert info["n_ground"] == 400 and info["n_unresolved"] == 0
    # a ground point finds itself: +0.0, to the bit
    assert (bits(hag[is_ground == 1]) == 0).all()
    # the same buffer without a mask: every point is ground, every height +0.0
    hag, _, info = gpu_hag(hip, pts, None, None, k=3, sq=storage)
    assert (bits(hag) == 0).all() and info["n_ground"] == 600
    # two different buffers, with and without a mask
    check(hip, pts[is_ground == 0], pts, is_ground, k=3, sq=storage, sg=storage, what="two buffers, mask")
    check(hip, pts[is_ground == 0], pts[is_ground == 1], None, k=3, sq=storage, sg=storage, what="two buffers, no mask")


def lattice(nx, ny, seed):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    pts = np.column_stack([gx.ravel(), gy.ravel(), rng.integers(0, 80, nx * ny) / 8.0])  # (multiples of 1/8: z + 100 and z + 200 are exact)
    return pts[rng.permutation(len(pts))]  # the tie rule is by buffer index: not the lattice's own order


@pytest.mark.gpu
@pytest.mark.parametrize("edge", [0.0, 0.5, 1.0, 2.0, 3.0])
def test_ties_on_a_lattice(hip, edge):
    """Ground on an integer lattice, queries on lattice points and cell centres: d2 takes few values (0, 1, 2, 4, 5, ... / 0.5, 2.5, 4.5, ...) and every
    one is shared by 4 or 8 ground points.  With edge 1 and 2 the lattice points lie ON cell borders; the k-th and (k + 1)-th candidate tie across a
    cell border (k = 2, 3 on a lattice point: the four at d2 = 1 are in four cells) and across a ring border (edge 0.5: they are two rings out)."""
    ground = lattice(13, 11, 12)
    on = np.array([[x, y, 50.0] for x in (0.0, 3.0, 6.0, 12.0) for y in (0.0, 5.0, 10.0)])
    centres = np.array([[x + 0.5, y + 0.5, 50.0] for x in (0.0, 4.0, 11.0) for y in (0.0, 6.0, 9.0)])
    q = np.concatenate([on, centres])
    for k in (1, 2, 3, 4, 5, 6, 9, 13):
        check(hip, q, ground, k=k, edge=edge, what=f"lattice k {k} edge {edge}")
    check(hip, q, ground, k=6, md=2.0, edge=edge, what="lattice, m2 = 4 is a tie class")
    # duplicated ground points with a different z, at a lower and at a higher index than their twin
    dup = np.concatenate([ground[100:120] + [0.0, 0.0, 100.0], ground, ground[:20] + [0.0, 0.0, 200.0]])
    for k in (1, 2, 5):
        check(hip, q, dup, k=k, edge=edge, what=f"duplicates k {k}")
    # query == ground with duplicates: the lower-indexed twin is the exact hit, so the higher-indexed one gets its height over it
    hag, _, _ = gpu_hag(hip, dup, None, None, k=2, edge=edge)
    assert_same_bits(hag, R.height_above_ground(dup, dup, None, 2)[0], "duplicates, same buffer")
    assert (hag[:20] == 0.0).all() and (hag[20 + 100:20 + 120] == -100.0).all() and (hag[-20:] == 200.0).all()


@pytest.mark.gpu
def test_max_distance_knife_edge(hip):
    # d2 = 25 exactly, and the next representable d2 above: 25 + 2^-48 = 5 * 5 + 2^-24 * 2^-24, exact in every step
    above = math.ldexp(1.0, -24)
    assert 25.0 + above * above == np.nextafter(25.0, INF)
    ground = np.array([[5.0, above, 1.0], [3.0, 4.0, 2.0], [-5.0, 0.0, 4.0], [0.0, 5.0, 8.0], [40.0, 40.0, 16.0]])
    q = np.array([[0.0, 0.0, 100.0]])
    for edge in (0.0, 1.0, 7.0, 100.0):
        for k in (1, 2, 3, 4):
            hag, gz, info = gpu_hag(hip, q, ground, k=k, md=5.0, edge=edge)
            want = R.height_above_ground(q, ground, None, k, 5.0)
            assert_same_bits(gz, want[1], f"knife edge k {k} edge {edge}")
            assert_same_bits(hag, want[0], f"knife edge k {k} edge {edge}")
        # the three at d2 == m2 are neighbours, the one a unit in the last place beyond is not: k = 4 uses three
        w = 1.0 / 25.0
        assert gz[0] == (w * 2.0 + w * 4.0 + w * 8.0) / (w + w + w)
        # a bound that leaves none
        hag, gz, info = gpu_hag(hip, q, ground, k=2, md=np.nextafter(5.0, 0.0), edge=edge)
        assert np.isnan(hag[0]) and np.isnan(gz[0]) and info["n_unresolved"] == 1 and info["n_ground"] == 5
    # fewer than k within the bound, on a cloud
    info = check(hip, queries(200, 13), terrain(300, 14), k=8, md=6.0, what="fewer than k")
    assert info["n_unresolved"] > 0  # (the margin around the square holds queries without any ground in reach)
    want = R.height_above_ground(queries(200, 13), terrain(300, 14), None, 8, 6.0)
    assert 0 < want[3] < 200


@pytest.mark.gpu
def test_grid_independence(hip):
    ground, q = terrain(1500, 15), queries(400, 16)
    mask = (np.arange(1500) % 4 != 0).astype(np.uint8)
    bufs = (make_buffer(hip, q, "H"), make_buffer(hip, ground, "V"))
    want = R.height_above_ground(q, ground, mask, 7)
    auto = gpu_hag(hip, q, ground, mask, k=7, bufs=bufs)
    assert_same_bits(auto[0], want[0], "automatic edge hag")
    assert_same_bits(auto[1], want[1], "automatic edge ground_z")
    e = auto[2]["cell_edge"]
    # the 3 x 3 cells around a query hold about 2k = 14 of the 1125 ground points: 9 e^2 * 1125 / area = 14
    assert 12.0 < 9.0 * e * e * auto[2]["n_ground"] / 1e4 < 16.0
    fine = gpu_hag(hip, q, ground, mask, k=7, edge=e / 8.0, bufs=bufs)
    single = gpu_hag(hip, q, ground, mask, k=7, edge=1000.0, bufs=bufs)
    for other in (fine, single):
        assert other[0].tobytes() == auto[0].tobytes() and other[1].tobytes() == auto[1].tobytes()
        assert (other[2]["n_ground"], other[2]["n_unresolved"]) == (auto[2]["n_ground"], auto[2]["n_unresolved"]) == (want[2], want[3])
    assert single[2]["dim"] == (1, 1) and single[2]["cell_edge"] == 1000.0
    assert fine[2]["cell_edge"] == e / 8.0
    member = ground[mask == 1]
    ext = member[:, :2].max(axis=0) - member[:, :2].min(axis=0)
    for info in (auto[2], fine[2]):
        assert info["dim"] == (int(ext[0] / info["cell_edge"]) + 1, int(ext[1] / info["cell_edge"]) + 1)
        assert info["origin"] == (member[:, 0].min(), member[:, 1].min())
    assert fine[2]["dim"][0] > 7 * auto[2]["dim"][0]


@pytest.mark.gpu
def test_grid_knife_edge(hip):
    # ground points exactly on cell borders and at the AABB's maximum (edge 1 and 2 over an integer lattice from 0 to 20), queries outside the AABB
    # on every side and corner, near and far
    ground = lattice(21, 21, 17)
    outside = np.array([[x, y, 5.0] for x in (-30.0, -0.5, 10.25, 20.0, 20.5, 55.0) for y in (-40.0, -0.25, 7.5, 20.0, 20.75, 61.0)])
    for edge in (1.0, 2.0, 0.0):
        for k in (1, 4, 9):
            info = check(hip, outside, ground, k=k, edge=edge, what=f"outside k {k} edge {edge}")
        if edge:
            assert info["dim"] == (int(20 / edge) + 1, int(20 / edge) + 1)
    # a query whose k-th neighbour lies several rings out while the nearer cells are empty: two far clusters and a little ground near the queries
    rng = np.random.default_rng(18)
    near = np.column_stack([50.0 + rng.random((3, 2)), rng.random(3)])
    far = np.concatenate([np.column_stack([rng.random((40, 2)) * 4.0 + c, rng.random(40)]) for c in ([0.0, 0.0], [96.0, 90.0])])
    ground = np.concatenate([near, far])
    q = np.column_stack([48.0 + rng.random((20, 2)) * 5.0, rng.random(20) * 9.0])
    for k in (2, 3, 4, 10):
        info = check(hip, q, ground, k=k, edge=1.0, what=f"several rings out k {k}")
    ext = ground[:, :2].max(axis=0) - ground[:, :2].min(axis=0)
    assert info["dim"] == (int(ext[0]) + 1, int(ext[1]) + 1) and min(info["dim"]) > 90
    # a far query that must walk to rmax with an unbounded distance: more neighbours asked for than the ground has, from a corner and from outside,
    # on a grid of 250 x 250 cells
    corners = np.array([[0.0, 0.0, 1.0], [100.0, 100.0, 2.0], [0.0, 100.0, 3.0], [100.0, 0.0, 4.0], [50.0, 50.0, 5.0]])
    q = np.array([[0.0, 0.0, 9.0], [100.0, 100.0, 9.0], [-500.0, 50.0, 9.0], [50.0, 1e4, 9.0], [49.9, 50.1, 9.0], [1e200, 0.0, 9.0]])
    info = check(hip, q, corners, k=8, edge=0.4, what="walk to rmax")
    assert info["dim"] == (int(100.0 / 0.4) + 1, int(100.0 / 0.4) + 1) and info["dim"][0] < 300


@pytest.mark.gpu
def test_degenerate_ground(hip):
    q = queries(90, 19, extent=10.0, margin=3.0)
    rng = np.random.default_rng(20)
    t = rng.random(50) * 10.0
    cases = {"one point": np.array([[4.0, 5.0, 6.0]]),
             "a vertical line": np.column_stack([np.full(50, 4.0), np.full(50, 5.0), t]),
             "a line along x": np.column_stack([t, np.full(50, 5.0), t * 0.5]),
             "a line along y": np.column_stack([np.full(50, 4.0), t, t * 0.25])}
    for name, ground in cases.items():
        for k in (1, 3, MAX_K):
            info = check(hip, q, ground, k=k, what=name)
        for edge in (0.3, 50.0):
            check(hip, q, ground, k=3, edge=edge, md=4.0, what=f"{name} edge {edge}")
        if name in ("one point", "a vertical line"):
            assert info["dim"] == (1, 1) and info["cell_edge"] == 1.0
        elif name == "a line along x":
            assert info["dim"][1] == 1 and info["dim"][0] > 1
        else:
            assert info["dim"][0] == 1 and info["dim"][1] > 1
    # a mask of zeros, only non-finite ground, an empty ground buffer: NaN everywhere, every finite query unresolved, a zero grid
    q[3, 0] = np.nan
    q[5, 2] = np.inf
    ground = cases["a line along x"]
    bad = ground.copy()
    bad[:, 1] = np.nan
    qb = make_buffer(hip, q, "H")
    for name, gb, mask in (("zero mask", make_buffer(hip, ground, "H"), np.zeros(50, dtype=np.uint8)), ("non-finite ground", make_buffer(hip, bad, "V"), None),
                           ("empty ground", _empty_buffer(hip), None)):
        for want_out in ("both", "hag", "gz"):
            hag, gz, info = gpu_hag(hip, None, None, mask, k=2, want=want_out, bufs=(qb, gb))
            for out in (hag, gz):
                assert out is None or np.isnan(out).all(), name
            assert info == {"n_ground": 0, "n_unresolved": 88, "origin": (0.0, 0.0), "cell_edge": 0.0, "dim": (0, 0)}, name


@pytest.mark.gpu
def test_non_finite_values(hip):
    ground, q = terrain(400, 21), queries(200, 22)
    for i, (col, v) in enumerate([(0, np.nan), (1, np.nan), (2, np.nan), (0, INF), (1, -INF), (2, INF), (2, -INF)]):
        ground[7 * i + 1, col] = v
        q[5 * i + 2, col] = v
    q[60] = [np.nan, np.nan, np.nan]
    for k, md, edge in ((1, INF, 0.0), (6, INF, 0.0), (6, 15.0, 2.5)):
        info = check(hip, q, ground, k=k, md=md, edge=edge, what=f"non-finite k {k}")
        assert info["n_ground"] == 393
    # the same cloud as its own ground: the non-finite points get NaN, and they are nobody's neighbour
    info = check(hip, ground, None, k=3, what="non-finite, same buffer")
    assert info["n_ground"] == 393 and info["n_unresolved"] == 0
    # squares that overflow: d2 = +inf is a distance like any other when the search is unbounded (weight 0, and 0 / 0 when every weight is)
    huge = np.array([[1e200, 0.0, 1.0], [-1e200, 3.0, 2.0], [1e160, 1e160, 3.0]])
    check(hip, huge, ground, k=4, what="overflowing squares")
    check(hip, huge, ground, k=4, md=1e150, what="overflowing squares, bounded")


@pytest.mark.gpu
def test_dense_cell(hip):
    """3000 ground points in one cell (a tight cluster and two far points that set the AABB), and all of them in the single cell of a large edge"""
    rng = np.random.default_rng(23)
    cluster = np.column_stack([50.0 + rng.random((3000, 2)) * 0.5, rng.random(3000)])
    ground = np.concatenate([cluster, [[0.0, 0.0, 0.0], [100.0, 100.0, 1.0]]])
    q = np.column_stack([49.5 + rng.random((100, 2)) * 1.5, rng.random(100) * 5.0])
    info = check(hip, q, ground, k=10, edge=1.0, what="dense cell")
    assert info["dim"] == (101, 101)
    check(hip, q, ground, k=MAX_K, edge=500.0, what="one cell for everything")


@pytest.mark.gpu
def test_outputs_and_repeatability(hip):
    ground, q = terrain(900, 24), queries(333, 25)
    mask = (np.arange(900) % 7 != 0).astype(np.uint8)
    bufs = (make_buffer(hip, q, "V"), make_buffer(hip, ground, "H"))
    want = R.height_above_ground(q, ground, mask, 10, 11.0)
    both = gpu_hag(hip, q, ground, mask, k=10, md=11.0, bufs=bufs)
    again = gpu_hag(hip, q, ground, mask, k=10, md=11.0, bufs=bufs)
    only_hag = gpu_hag(hip, q, ground, mask, k=10, md=11.0, want="hag", bufs=bufs)
    only_gz = gpu_hag(hip, q, ground, mask, k=10, md=11.0, want="gz", bufs=bufs)
    assert_same_bits(both[0], want[0], "hag")
    assert_same_bits(both[1], want[1], "ground_z")
    assert only_hag[1] is None and only_gz[0] is None
    assert again[0].tobytes() == both[0].tobytes() == only_hag[0].tobytes() and again[1].tobytes() == both[1].tobytes() == only_gz[1].tobytes()
    for r in (both, again, only_hag, only_gz):
        assert (r[2]["n_ground"], r[2]["n_unresolved"]) == (want[2], want[3]) and r[2] == both[2]
    assert want[3] > 0
    # the optional host pointers may all be absent
    import torch
    out = torch.zeros(333, dtype=torch.float64, device="cuda")
    m = device_bytes(mask)
    hip.height_above_ground_device(bufs[0]._h, bufs[1]._h, C.c_void_p(m.data_ptr()), 10, 11.0, 0.0, C.c_void_p(out.data_ptr()), None, None, None, None, None)
    assert out.cpu().numpy().tobytes() == both[0].tobytes()


@pytest.mark.gpu
def test_python_wrappers(hip):
    ground, q = terrain(500, 26), queries(150, 27)
    mask = (np.arange(500) % 3 != 0).astype(np.uint8)
    qb, gb = make_buffer(hip, q, "H"), make_buffer(hip, ground, "H")
    want = R.height_above_ground(q, ground, mask, 4)
    hag = alg.height_above_ground(qb, mask, k=4, ground=gb)
    assert hag.dtype == np.float64
    assert_same_bits(hag, want[0], "numpy mask")
    on_device = device_bytes(mask)
    hag, gz = alg.height_above_ground(qb, on_device.data_ptr(), k=4, ground=gb, return_ground_z=True)
    assert_same_bits(hag, want[0], "device mask")
    assert_same_bits(gz, want[1], "device mask ground_z")
    with pytest.raises(ValueError):
        alg.height_above_ground(qb, mask[:-1], k=4, ground=gb)
    # ground_mask None: Classification == 2 of the ground buffer
    pts = np.concatenate([ground, q])
    classes = np.concatenate([np.where(mask == 1, 2, 1), np.full(len(q), 5)]).astype(np.uint8)
    buf = _classified_buffer(hip, pts, HashMapBuffer, classes)
    want = R.height_above_ground(pts, pts, classes == 2, 4, 25.0)
    assert_same_bits(alg.height_above_ground(buf, k=4, max_distance=25.0), want[0], "Classification == 2")
    empty = _classified_buffer(hip, np.zeros((0, 3)), HashMapBuffer, np.zeros(0, dtype=np.uint8))
    assert alg.height_above_ground(empty).shape == (0,) and alg.normalize_height(empty) == 0


def _classified_buffer(hip, pts, kind, classes):
    layout = PointLayout.from_attributes([A.POSITION_3D, A.INTENSITY, A.CLASSIFICATION], api=hip)
    buf = kind.new_from_layout(layout)
    n = len(pts)
    buf.resize(n)
    if n:
        buf.set_attribute_range(A.POSITION_3D, range(0, n), np.ascontiguousarray(pts))
        buf.set_attribute_range(A.INTENSITY, range(0, n), (np.arange(n) * 7 % 65521).astype(np.uint16))
        buf.set_attribute_range(A.CLASSIFICATION, range(0, n), classes)
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [HashMapBuffer, VectorBuffer])
@pytest.mark.parametrize("n", [1, MASK_POINTS - 1, MASK_POINTS, MASK_POINTS + 1, 3 * MASK_POINTS + 5])
def test_u8_equals_mask(hip, kind, n):
    import torch
    classes = (np.arange(n) * 5 % 7).astype(np.uint8)
    buf = _classified_buffer(hip, terrain(n, 28), kind, classes)
    for value in (2, 0, 6, 200):  # (no point has class 200)
        m = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
        alg.classification_mask(buf, value, m.data_ptr())
        torch.cuda.synchronize()
        got = m.cpu().numpy()
        assert np.array_equal(got[:n], (classes == value).astype(np.uint8)) and (got[n:] == 9).all()
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), classes)  # the attribute is only read


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [HashMapBuffer, VectorBuffer])
def test_classification_mask_inverts_classify_ground(hip, kind):
    import torch
    scene = _scene_module().scene(4000, seed=3)[0]
    params = alg.PmfParameters(1.0, 17.0, 1.0, 0.5, 1.2)
    buf = _classified_buffer(hip, scene, kind, np.full(len(scene), 7, dtype=np.uint8))
    want_mask, want_count = alg.ground_mask(buf, params)
    assert alg.classify_ground(buf, params) == want_count
    m = torch.zeros(len(scene), dtype=torch.uint8, device="cuda")
    alg.classification_mask(buf, 2, m.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), want_mask) and 0 < want_count < len(scene)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [HashMapBuffer, VectorBuffer])
def test_normalize_height(hip, kind):
    pts = np.concatenate([terrain(600, 29), queries(200, 30)])
    classes = np.concatenate([np.full(600, 2), np.full(200, 1)]).astype(np.uint8)
    pts[610, 2] = np.nan
    order = np.random.default_rng(31).permutation(800)
    pts, classes = pts[order], classes[order]
    want = R.height_above_ground(pts, pts, classes == 2, 5, 8.0)
    buf = _classified_buffer(hip, pts, kind, classes)
    assert alg.normalize_height(buf, k=5, max_distance=8.0) == want[3] and want[3] > 0
    after = buf.view_attribute(A.POSITION_3D)
    assert_same_bits(after[:, 2], want[0], "z after normalize_height")
    assert after[:, :2].tobytes() == np.ascontiguousarray(pts[:, :2]).tobytes()
    assert np.array_equal(buf.view_attribute(A.CLASSIFICATION), classes)
    assert (bits(after[classes == 2, 2]) == 0).all()  # the ground itself: +0.0


def _scene_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("classify_ground_scene", os.path.join(root, "examples", "classify_ground.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_example_runs(hip):
    """examples/height_above_ground.py: every planted object comes out once, and its tallest height above the ground is the height it was built
    with, up to what the terrain varies by under and around it.  The ground elevation under a roof point is a convex combination of ground points
    that lie within the box's half-sizes plus the reach of the 10 nearest ground points (below 1.5 m at 6 points per square metre) of the box's
    centre; the terrain's slope is at most 0.02 + 1.5 / 15 = 0.12 along x and 1.5 / 18 along y, its noise 2 cm (0.1 is five sigma)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("height_above_ground", os.path.join(root, "examples", "height_above_ground.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(60000)
    assert result["n_unresolved"] == 0
    assert sorted(f["object"] for f in result["found"]) == list(range(result["objects_planted"]))
    for f in result["found"]:
        _, _, sx, sy, h = mod.scene_module.OBJECTS[f["object"]]
        assert f["built"] == mod.scene_module.CLEAR + h
        bound = 0.12 * (sx / 2 + 1.5) + (1.5 / 18.0) * (sy / 2 + 1.5) + 0.1
        assert abs(f["tallest"] - f["built"]) <= bound, (f, bound)
