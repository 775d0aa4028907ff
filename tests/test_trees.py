"""Individual trees (pst_tree_tops_device, pst_segment_trees_device): the numpy restatement tests/trees_ref.py on hand-built cases, one per
rule of the definition; every check the host answers without a device; and on the GPU masks, index lists, ids, counts and scalar counts
against the restatement, all EQUAL: no tolerance appears anywhere."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import trees_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

P, S, Q, BOUNDS_POINTS = 256, 4, 64, 4096  # asserted against pst_trees_kernel_shape below: the parametrisations need them at collection time
WAVE = 64
STORAGES = ["H", "V", "packedH", "packedV", "external", "sliceH", "sliceV"]  # the list of test_hag.py
INF = float("inf")
NAN = float("nan")
NO_TREE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIABLE = (1.5, 0.1, 1.0, 5.0)  # radii


def up(v, ulps=1):
    for _ in range(ulps):
        v = np.nextafter(v, INF)
    return float(v)


def down(v, ulps=1):
    for _ in range(ulps):
        v = np.nextafter(v, -INF)
    return float(v)


# ---------------------------------------------------------------------------------------------------------------------------------- scenes

def stand(n, seed, extent, pitch=10.0, noise=0.0):
    """(points, trunks): n points uniform over [0, extent)^2 under a stand of paraboloid crowns, heights 8 - 20 m and crown radius a quarter
    of the height, on a lattice of `pitch` jittered by +-1 m; the height of a point is the highest crown over it, on ground of 0 - 0.3 m"""
    rng = np.random.default_rng(seed)
    k = int(extent // pitch)
    gx, gy = np.meshgrid((np.arange(k) + 0.5) * pitch, (np.arange(k) + 0.5) * pitch)
    trunks = np.column_stack([gx.ravel(), gy.ravel()]) + rng.uniform(-1.0, 1.0, (k * k, 2))
    H = rng.uniform(8.0, 20.0, k * k)
    xy = rng.random((n, 2)) * extent
    # one point exactly on every trunk: the planted tree's apex
    xy[:min(n, k * k)] = trunks[:n]
    h = rng.random(n) * 0.3
    for c0 in range(0, n, 20000):
        sl = slice(c0, c0 + 20000)
        d2 = ((xy[sl, None, :] - trunks[None, :, :]) ** 2).sum(axis=2)
        crown = H[None, :] * (1.0 - d2 / (0.25 * H[None, :]) ** 2)
        h[sl] = np.maximum(h[sl], crown.max(axis=1))
    if noise:
        h = h + rng.normal(0.0, noise, n)
    order = rng.permutation(n)
    return np.column_stack([xy, h])[order], trunks, H


def canopy(n, seed):
    """a closed, noisy canopy over about a point per 0.2 m^2 -- a tree per 4 m, so the crowns overlap and nearly every point is a candidate:
    every phase has work"""
    return stand(n, seed, max(4.0, float(np.sqrt(n / 5.0))), pitch=4.0, noise=0.3)[0]


# ------------------------------------------------------------------------------------------------------------ the restatement, by hand

def tops_of(pts, window, min_height, **kw):
    top, idx, nc = R.tree_tops(np.asarray(pts, dtype=np.float64), window, min_height, **kw)
    return top.tolist(), idx.tolist(), nc


def test_restatement_window_edge_is_inclusive():
    fixed = (5.0, 0.0, 5.0, 5.0)
    assert tops_of([[0, 0, 10], [5, 0, 11]], fixed, 2.0)[0] == [0, 1]                 # d2 == r*r: dominated
    assert tops_of([[0, 0, 10], [up(5.0), 0, 11]], fixed, 2.0)[0] == [1, 1]           # one ulp beyond: not
    assert tops_of([[0, 0, 10], [3, 4, 11]], fixed, 2.0)[0] == [0, 1]                 # 9 + 16 == 25
    assert tops_of([[0, 0, 10], [3, up(4.0), 11]], fixed, 2.0)[0] == [1, 1]


def test_restatement_tie_goes_to_the_lower_index():
    fixed = (5.0, 0.0, 5.0, 5.0)
    assert tops_of([[0, 0, 10], [1, 0, 10], [2, 0, 10]], fixed, 2.0)[0] == [1, 0, 0]
    assert tops_of([[0, 0, -0.0], [1, 0, 0.0]], fixed, -1.0)[0] == [1, 0]             # the two zeros are equal
    assert tops_of([[0, 0, 0.0], [1, 0, -0.0]], fixed, -1.0)[0] == [1, 0]


def test_restatement_variable_window_is_asymmetric():
    # r = h / 10: the tall point's window (r = 2) reaches the low one, the low one's (r = 1) does not reach the tall one
    w = (0.0, 0.1, 0.0, INF)
    top, idx, _ = tops_of([[0, 0, 10], [1.5, 0, 20]], w, 2.0)
    assert top == [1, 1] and idx == [1, 0]
    # b < 0: the LOW point has the wide window and sees the tall one
    assert tops_of([[0, 0, 10], [1.5, 0, 20]], (3.0, -0.1, 0.0, INF), 2.0)[0] == [0, 1]
    # the clamps: a + b*h below r_min, above r_max
    assert tops_of([[0, 0, 1], [2, 0, 3]], (0.0, 0.1, 2.0, 4.0), 0.0)[0] == [0, 1]    # r = 2 at both
    assert tops_of([[0, 0, 100], [up(4.0), 0, 200]], (0.0, 0.1, 2.0, 4.0), 0.0)[0] == [1, 1]


def test_restatement_candidate_floor_mask_and_non_finite():
    fixed = (5.0, 0.0, 5.0, 5.0)
    top, idx, nc = tops_of([[0, 0, 2.0], [1, 0, down(2.0)], [30, 0, 1.0]], fixed, 2.0)
    assert top == [1, 0, 0] and nc == 1                                               # h == min_height is a candidate, an ulp below is not
    # a point below the floor dominates nobody; a masked or non-finite point neither
    pts = [[0, 0, 10], [1, 0, 50], [2, 0, 60], [3, NAN, 70], [NAN, 0, 70], [4, 0, INF]]
    top, idx, nc = tops_of(pts, fixed, 2.0, mask=[1, 0, 1, 1, 1, 1])
    assert top == [0, 0, 1, 0, 0, 0] and nc == 2
    assert tops_of(pts[:2], fixed, 55.0)[0] == [0, 0]
    # a column replaces z, which is then not looked at
    top, idx, nc = tops_of([[0, 0, NAN], [1, 0, 99]], fixed, 2.0, heights=[5.0, 3.0])
    assert top == [1, 0] and nc == 2
    # a radius of 0 keeps exact duplicates inside the window
    assert tops_of([[1, 1, 5], [1, 1, 6], [1, 1, 6], [up(1.0), 1, 9]], (0.0, 0.0, 0.0, 0.0), 2.0)[0] == [0, 1, 0, 1]


def test_restatement_numbering():
    fixed = (1.0, 0.0, 1.0, 1.0)
    pts = [[0, 0, 5], [10, 0, 9], [20, 0, 5], [30, 0, 9], [40, 0, 7]]
    assert tops_of(pts, fixed, 2.0)[1] == [1, 3, 4, 0, 2]                             # descending height, ties ascending index
    assert R.number_trees([1, 1, 1], np.array([0.0, -0.0, 0.0])).tolist() == [0, 1, 2]


def ids_of(pts, top_mask, factor, exclusion, min_height, **kw):
    ids, counts, total, trees = R.segment_trees(np.asarray(pts, dtype=np.float64), top_mask, factor, exclusion, min_height, **kw)
    assert counts.sum() == total == (ids != NO_TREE).sum()
    return ids.tolist(), counts.tolist()


def test_restatement_crowns():
    # nearest first, THEN the test: point 2 is nearest to the small tree, outside its crown, inside the big one's -- and gets nothing
    pts = [[0, 0, 20], [10, 0, 4], [7.5, 0, 3]]
    ids, counts = ids_of(pts, [1, 1, 0], 1.0, 0.0, 2.0)
    assert ids == [0, 1, NO_TREE] and counts == [1, 1]
    # both knife edges: rc = 0.5 * 0.5 * 20 = 5, exclusion * H = 0.25 * 20 = 5
    base = [[0, 0, 20]]
    assert ids_of(base + [[5, 0, 5]], [1, 0], 0.5, 0.25, 2.0)[0] == [0, 0]
    assert ids_of(base + [[up(5.0), 0, 5]], [1, 0], 0.5, 0.25, 2.0)[0] == [0, NO_TREE]
    assert ids_of(base + [[3, 4, down(5.0)]], [1, 0], 0.5, 0.25, 2.0)[0] == [0, NO_TREE]
    assert ids_of(base + [[3, 4, 5]], [1, 0], 0.5, 0.25, 2.0)[0] == [0, 0]
    # equidistant tops: the smaller buffer index, whatever its number
    ids, _ = ids_of([[0, 0, 10], [2, 0, 30], [1, 0, 5], [1, 7, 5]], [1, 1, 0, 0], 10.0, 0.0, 2.0)
    assert ids == [1, 0, 1, 1]
    # min_height, the mask, a top below min_height (labels others, not itself), a non-finite top (no tree), factor 0
    ids, counts = ids_of([[0, 0, 1.5], [1, 0, 3], [1, 0, 1], [NAN, 0, 9], [2, 0, 3]], [1, 0, 0, 1, 0], 100.0, 0.0, 2.0, mask=[1, 1, 1, 1, 0])
    assert ids == [NO_TREE, 0, NO_TREE, NO_TREE, NO_TREE] and counts == [1]
    assert ids_of([[0, 0, 10], [0, 0, 9], [1, 0, 9]], [1, 0, 0], 0.0, 0.0, 2.0)[0] == [0, 0, NO_TREE]
    assert ids_of([[0, 0, 10], [1, 0, 9]], [0, 0], 1.0, 0.0, 2.0) == ([NO_TREE, NO_TREE], [])


def test_the_scene_of_the_issue_has_its_planted_trees():
    """20 011 points, 36 crowns: both windows of the issue find every planted tree and nothing else, each top on its trunk's apex point"""
    pts, trunks, H = stand(20011, 1, 60.0)
    assert len(trunks) == 36
    for window in (VARIABLE, (3.0, 0.0, 3.0, 3.0)):
        top, idx, nc = R.tree_tops(pts, window, 2.0)
        assert len(idx) == 36 and nc > 3000
        assert sorted(map(tuple, pts[idx.astype(np.int64), :2].tolist())) == sorted(map(tuple, trunks.tolist()))
    assert len(R.tree_tops(pts, (0.25, 0.0, 0.25, 0.25), 2.0)[1]) > 36  # windows too small
    ids, counts, total, _ = R.segment_trees(pts, top, 0.6, 0.3, 2.0)
    assert 5000 < total <= (pts[:, 2] >= 2.0).sum() and counts.min() >= 20 and len(counts) == 36


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _empty_buffer(hip, dtype=T.Vec3f64):
    return HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def test_kernel_shape(hip):
    assert alg.trees_kernel_shape(hip) == {"points_per_block": P, "survivors_per_block": S, "queries_per_block": Q, "bounds_points_per_block": BOUNDS_POINTS}
    one = C.c_uint32()
    hip.trees_kernel_shape(None, None, C.byref(one), None)  # each pointer is optional
    assert one.value == Q
    hip.trees_kernel_shape(None, None, None, None)
    assert _code(lambda: hip.trees_phase_times(None)) == 1
    assert _code(lambda: hip.trees_work(None)) == 1
    assert len(alg.trees_phase_times(hip)) == 4 and set(alg.trees_work(hip)) == {"candidates", "survivors", "far_tested"}


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments and invalid parameters: the same status with or without a device, because no device is looked for."""
    buf = _empty_buffer(hip)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails before that
    nc, nt, me, dim = C.c_uint64(7), C.c_uint64(7), (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 2)(1, 1)

    def tops(b=buf._h, mh=2.0, w=(1.5, 0.1, 1.0, 5.0), edge=0.0, mask=fake):
        return hip.tree_tops_device(b, None, None, mh, (C.c_double * 4)(*w) if w is not None else None, edge, mask, None, 0, C.byref(nc), C.byref(nt), me, dim)
    assert _code(lambda: tops(b=None)) == 1
    assert _code(lambda: tops(w=None)) == 1
    for mh in (NAN, INF, -INF):
        assert _code(lambda: tops(mh=mh)) == 1
    for w in ((NAN, 0, 1, 2), (INF, 0, 1, 2), (0, NAN, 1, 2), (0, -INF, 1, 2), (0, 0, -1, 2), (0, 0, NAN, 2), (0, 0, INF, INF), (0, 0, 3, 2), (0, 0, 1, NAN)):
        assert _code(lambda: tops(w=w)) == 1
    for edge in (-1.0, NAN, INF, -INF):
        assert _code(lambda: tops(edge=edge)) == 1
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(lambda: tops(b=f32._h)) == 4
    with pytest.raises(PasturePanic):
        tops(b=f32._h)
    assert _code(lambda: tops(b=f32._h, mh=NAN)) == 1  # the parameters come before the layout
    # an empty buffer: PST_OK on the host, nothing written, zeros in the counts and the grid; every optional pointer absent; r_max = +inf, b < 0
    assert tops() == 0 and tops(mask=None) == 0 and tops(w=(0, -1, 0, INF)) == 0
    assert (nc.value, nt.value, list(me), list(dim)) == (0, 0, [0.0, 0.0, 0.0], [0, 0])
    assert hip.tree_tops_device(buf._h, None, None, 2.0, (C.c_double * 4)(3, 0, 3, 3), 5.0, None, None, 0, None, None, None, None) == 0

    ntr, nl = C.c_uint64(7), C.c_uint64(7)

    def seg(b=buf._h, mh=2.0, f=0.6, ex=0.3, edge=0.0):
        return hip.segment_trees_device(b, None, None, fake, mh, f, ex, edge, fake, None, 0, C.byref(ntr), C.byref(nl))
    assert _code(lambda: seg(b=None)) == 1
    for mh in (NAN, INF):
        assert _code(lambda: seg(mh=mh)) == 1
    for f in (-0.1, NAN, INF):
        assert _code(lambda: seg(f=f)) == 1
    for ex in (-0.1, 1.1, NAN):
        assert _code(lambda: seg(ex=ex)) == 1
    for edge in (-1.0, NAN, INF):
        assert _code(lambda: seg(edge=edge)) == 1
    assert _code(lambda: seg(b=f32._h)) == 4
    assert seg() == 0 and seg(f=0.0, ex=0.0) == 0 and seg(ex=1.0) == 0
    assert (ntr.value, nl.value) == (0, 0)
    assert hip.segment_trees_device(buf._h, None, None, None, 2.0, 0.6, 0.3, 0.0, None, None, 0, None, None) == 0
    # the Python layer on an empty buffer
    t = alg.tree_tops(buf, window=3.0)
    assert (t.n_tops, t.n_candidates, len(t.indices), len(t.heights), len(t.mask)) == (0, 0, 0, 0, 0)
    s = alg.segment_trees(buf, t)
    assert (s.n_trees, s.n_labelled, len(s.tree_id), len(s.counts)) == (0, 0, 0, 0)
    assert alg._window_radii(6.0) == (3.0, 0.0, 3.0, 3.0) and alg._window_radii((3.0, 0.2, 2.0, 10.0)) == (1.5, 0.1, 1.0, 5.0)


_NO_DEVICE_SCRIPT = r"""
import numpy as np
import pasture_amd as pa
from pasture_amd import algorithms as alg
from pasture_amd.buffers import ExternalMemoryBuffer
from pasture_amd.layout import PointLayout, attributes as A
hip = pa.product_api()
points = np.arange(30.0).reshape(10, 3)  # ten points in host memory
buf = ExternalMemoryBuffer(points.ctypes.data, PointLayout.from_attributes([A.POSITION_3D], api=hip), nbytes=points.nbytes)
assert buf.len() == 10
calls = [lambda: alg.tree_tops_device(buf, (3.0, 0.0, 3.0, 3.0), 2.0, 8), lambda: alg.segment_trees_device(buf, 8, 8)]
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
    """Without a GPU both calls on a NON-EMPTY buffer are PST_ERR_NO_DEVICE, never a CPU path (caller's host memory wrapped as a buffer with
    PST_EXTERNAL_UNCHECKED, read once per process: hence the child process)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    env = dict(os.environ, PST_EXTERNAL_UNCHECKED="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE_SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"codes {[(21, True)] * 2}" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------------------- GPU helpers

def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def gpu_tops(hip, pts, window, min_height, heights=None, mask=None, edge=0.0, storage="H", capacity=None, buf=None):
    """(top mask, indices in tree order or None, info) through the C entry point"""
    import torch
    buf = make_buffer(hip, pts, storage) if buf is None else buf
    n = buf.len()
    h = dev(heights, np.float64) if heights is not None else None
    m = dev(mask, np.uint8) if mask is not None else None
    top = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    cap = n if capacity is None else capacity
    idx = torch.full((max(cap, 1),), 0x2B2B2B2B, dtype=torch.int32, device="cuda") if cap >= 0 else None
    info = alg.tree_tops_device(buf, window, min_height, top.data_ptr(), h.data_ptr() if h is not None and n else 0, m.data_ptr() if m is not None and n else 0, edge,
                                idx.data_ptr() if idx is not None else 0, max(cap, 0))
    torch.cuda.synchronize()
    out_idx = idx.cpu().numpy().view(np.uint32)[:info["n_tops"]] if idx is not None else None
    return top.cpu().numpy()[:n], out_idx, info


def check_tops(hip, pts, window, min_height, what="", edges=(0.0,), want=None, **kw):
    """the device against the restatement at every edge of `edges`; returns (the restatement's result, the last info)"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    want = R.tree_tops(pts, window, min_height, heights=kw.get("heights"), mask=kw.get("mask")) if want is None else want
    info = None
    for edge in edges:
        top, idx, info = gpu_tops(hip, pts, window, min_height, edge=edge, **kw)
        assert np.array_equal(top, want[0]), f"{what} edge {edge}: top mask differs at {np.flatnonzero(top != want[0])[:8]}"
        assert np.array_equal(idx, want[1]), f"{what} edge {edge}: the tree order differs"
        assert (info["n_candidates"], info["n_tops"]) == (want[2], len(want[1])), f"{what} edge {edge}: counts {info}"
    return want, info


def gpu_crowns(hip, pts, top_mask, factor, exclusion, min_height, heights=None, mask=None, edge=0.0, storage="H", capacity=None):
    import torch
    buf = make_buffer(hip, pts, storage)
    n = buf.len()
    h = dev(heights, np.float64) if heights is not None else None
    m = dev(mask, np.uint8) if mask is not None else None
    t = dev(top_mask, np.uint8)
    assert len(top_mask) == n
    ids = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    cap = n if capacity is None else capacity
    counts = torch.full((max(cap, 1),), 7, dtype=torch.int32, device="cuda")
    info = alg.segment_trees_device(buf, t.data_ptr(), ids.data_ptr(), factor, exclusion, min_height, h.data_ptr() if h is not None else 0,
                                    m.data_ptr() if m is not None else 0, edge, counts.data_ptr(), cap)
    torch.cuda.synchronize()
    return ids.cpu().numpy().view(np.uint32)[:n], counts.cpu().numpy().view(np.uint32)[:info["n_trees"]], info


def check_crowns(hip, pts, top_mask, factor, exclusion, min_height, what="", edges=(0.0,), **kw):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    want = R.segment_trees(pts, top_mask, factor, exclusion, min_height, heights=kw.get("heights"), mask=kw.get("mask"))
    for edge in edges:
        ids, counts, info = gpu_crowns(hip, pts, top_mask, factor, exclusion, min_height, edge=edge, **kw)
        assert np.array_equal(ids, want[0]), f"{what} edge {edge}: ids differ at {np.flatnonzero(ids != want[0])[:8]}"
        assert np.array_equal(counts, want[1]), f"{what} edge {edge}: counts differ"
        assert (info["n_trees"], info["n_labelled"]) == (len(want[1]), want[2]) and counts.sum() == info["n_labelled"], f"{what} edge {edge}: {info}"
    return want


def four_edges(hip, pts, window, min_height, **kw):
    """the automatic edge, an eighth of it, one cell for everything and 10^-3 of the window"""
    auto = gpu_tops(hip, pts, window, min_height, **kw)[2]["cell_edge"]
    r = float(R.window_radius(np.float64(np.nanmax(np.abs(np.asarray(pts)[:, 2]))), window))
    return (0.0, auto / 8.0, 1e7, max(r, 1e-3) * 1e-3)


# ------------------------------------------------------------------------------------------------------------------------------ GPU tests

SEAMS = sorted({0, 1, 2, S - 1, S, S + 1, WAVE - 1, WAVE, WAVE + 1, P - 1, P, P + 1, BOUNDS_POINTS - 1, BOUNDS_POINTS, BOUNDS_POINTS + 1, 2 * BOUNDS_POINTS + 3, 12007})


@pytest.mark.gpu
@pytest.mark.parametrize("n", SEAMS)
def test_lengths_around_the_seams(hip, n):
    """every length at which a kernel's last block, wave or block partial is empty, full or one over: tops and crowns on a noisy canopy"""
    pts = canopy(n, 100 + n)
    for window in (VARIABLE, (1.0, 0.0, 1.0, 1.0)):
        want, info = check_tops(hip, pts, window, 2.0, what=f"n {n} window {window}")
        if n >= BOUNDS_POINTS:
            work = alg.trees_work(hip)
            assert 0 < work["survivors"] < work["candidates"] and len(want[1]) > 0  # (every phase did have work)
    top = R.tree_tops(pts, VARIABLE, 2.0)[0]
    check_crowns(hip, pts, top, 0.6, 0.3, 2.0, what=f"n {n}")


@pytest.mark.gpu
def test_nobody_survives_the_near_pass(hip):
    pts = canopy(3000, 7)
    check_tops(hip, pts, VARIABLE, 2.0, edges=(1e6,), what="one cell")  # every box lies inside the 3 x 3 cells: the near pass decides all
    assert alg.trees_work(hip)["survivors"] == 0 and alg.trees_work(hip)["candidates"] > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("k", [WAVE - 1, WAVE, WAVE + 1, 700])
def test_exactly_k_survive_the_near_pass(hip, k):
    """k isolated points 10 m apart with a window of 3 m and cells of 1 m: nobody near them, a box of 7 x 7 cells -- all of them go to the far
    pass and all are tops.  Every third has a lower companion 0.1 m away, which the near pass rejects."""
    rng = np.random.default_rng(k)
    side = int(np.ceil(np.sqrt(k)))
    iso = np.array([[10.0 * (i % side), 10.0 * (i // side), 5.0 + rng.random()] for i in range(k)])
    low = iso[::3] + np.array([0.1, 0.05, -1.0])
    for pts, survivors in ((iso, k), (np.concatenate([low, iso]), k)):
        want, _ = check_tops(hip, pts, (3.0, 0.0, 3.0, 3.0), 2.0, edges=(1.0,), what=f"{k} isolated")
        assert alg.trees_work(hip) == {"candidates": len(pts), "survivors": survivors, "far_tested": 0}
        assert len(want[1]) == k


def nudge(v, away_positive, ulps):
    return up(v, ulps) if away_positive else down(v, ulps)


def knife_cloud():
    """independent pairs 1000 m apart around a window of r = 5: a dominator exactly on the edge, and one and two ulps OF ITS OWN COORDINATE
    beyond it (the differences stay exact), in the four directions and on the diagonals (3, 4, 5); and a pair of equal heights likewise"""
    pts, k = [], 0
    for dx, dy in ((5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (-3, 4), (3, -4), (-4, -3)):
        for beyond in (0, 1, 2):
            for x0, (hi, hj) in ((1000.0 * k, (10.0, 11.0)), (1000.0 * k + 100.0, (10.0, 10.0))):
                y0 = 500.0 * (k % 3)
                xj = nudge(x0 + dx, dx > 0, beyond) if dx else x0
                yj = nudge(y0 + dy, dy > 0, beyond) if dy and not dx else y0 + dy
                pts += [[xj, yj, hj], [x0, y0, hi]]  # the would-be dominator has the lower index
            k += 1
    return np.array(pts)


@pytest.mark.gpu
def test_window_knife_edges_to_the_ulp(hip):
    pts = knife_cloud()
    fixed = (5.0, 0.0, 5.0, 5.0)
    # edges that put the window's end on a cell boundary (5, 2.5, 1, 1/3 of it) and beside one
    want, _ = check_tops(hip, pts, fixed, 2.0, edges=(0.0, 5.0, 2.5, 1.0, 5.0 / 3.0, 0.7, 1e7), what="knife")
    top = want[0].reshape(-1, 4)
    assert top[0::3, 1].tolist() == [0] * 8 and top[1::3, 1].tolist() == [1] * 8 and top[2::3, 1].tolist() == [1] * 8  # (the cases are what they claim)
    assert top[0::3, 3].tolist() == [0] * 8 and top[1::3, 3].tolist() == [1] * 8 and top[:, 0].all() and top[:, 2].all()
    # the same at the origin, where one ulp of the coordinate is one ulp of r
    for dx, dy in ((5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (-4, -3)):
        for beyond in (0, 1):
            pair = [[np.sign(dx) * up(abs(dx), beyond) if dx else 0.0, np.sign(dy) * up(abs(dy), beyond) if dy else 0.0, 11.0], [0.0, 0.0, 10.0]]
            w2, _ = check_tops(hip, pair, fixed, 2.0, edges=(0.0, 5.0, 1.0), what=f"origin {dx} {dy} +{beyond}")
            assert w2[0].tolist() == [1, beyond]
    # the radius at both clamps, to the ulp: r = a + b*h with a + b*h == r_min and == r_max
    w = (0.0, 0.5, 5.0, 5.0)
    check_tops(hip, pts, w, 2.0, edges=(0.0, 1.0), what="clamped", want=want)
    # h == min_height is a candidate, an ulp below is not (and then dominates nobody)
    floor = np.array([[0, 0, 3.0], [1, 0, down(3.0)], [50, 0, down(3.0)], [51, 0, 2.0], [100, 0, 3.0], [101, 0, up(3.0)]])
    want, _ = check_tops(hip, floor, fixed, 3.0, what="floor")
    assert want[0].tolist() == [1, 0, 0, 0, 0, 1] and want[2] == 3


@pytest.mark.gpu
def test_radius_zero_and_exact_duplicates(hip):
    rng = np.random.default_rng(5)
    base = np.column_stack([rng.integers(0, 20, (300, 2)).astype(np.float64), rng.integers(3, 6, 300).astype(np.float64)])  # many shared xy and h
    want, _ = check_tops(hip, base, (0.0, 0.0, 0.0, 0.0), 2.0, edges=(0.0, 0.5, 1e6), what="r 0")
    assert 0 < len(want[1]) < 300


@pytest.mark.gpu
@pytest.mark.parametrize("window", [VARIABLE, (3.0, 0.0, 3.0, 3.0), (4.0, -0.1, 0.5, 4.0)])
def test_grid_independence(hip, window):
    pts = canopy(5000, 11)
    edges = four_edges(hip, pts, window, 2.0)
    want, _ = check_tops(hip, pts, window, 2.0, edges=edges, what=f"window {window}")
    check_crowns(hip, pts, want[0], 0.6, 0.3, 2.0, edges=(0.0, 0.4, 1e7, 3e-3 * 6.0), what="crowns")


@pytest.mark.gpu
def test_dense_cell_and_plateau(hip):
    rng = np.random.default_rng(3)
    dense = np.column_stack([rng.random((5000, 2)) * 0.5, rng.integers(10, 14, 5000).astype(np.float64)])  # one cell, heights 10 .. 13 shared by many
    dense[100:140] = dense[7]   # exact duplicates, equal h
    dense[7, 2] = dense[100:140, 2] = 13.0
    want, _ = check_tops(hip, dense, (3.0, 0.0, 3.0, 3.0), 2.0, edges=(0.0, 1e6), what="dense")
    assert want[1].tolist() == [int(np.flatnonzero(dense[:, 2] == 13.0)[0])]  # only the lowest index of the tallest
    gx, gy = np.meshgrid(np.arange(64.0), np.arange(64.0))
    plateau = np.column_stack([gx.ravel(), gy.ravel(), np.full(4096, 7.0)])
    want, _ = check_tops(hip, plateau, (1.5, 0.0, 1.5, 1.5), 2.0, edges=(0.0, 1.0), what="plateau")
    assert want[0][0] == 1 and 0 < len(want[1]) < 4096 // 4


@pytest.mark.gpu
def test_inputs_column_mask_non_finite_negative_and_zeros(hip):
    pts = canopy(3000, 21)
    h = pts[:, 2].copy()
    # the column against the same values in z: z is not consulted, not even when it is not finite
    junk = pts.copy()
    junk[:, 2] = np.where(np.arange(3000) % 2 == 0, NAN, -INF)
    want = R.tree_tops(pts, VARIABLE, 2.0)
    check_tops(hip, junk, VARIABLE, 2.0, heights=h, want=want, what="column")
    check_crowns(hip, junk, want[0], 0.6, 0.3, 2.0, heights=h, what="column crowns")
    assert np.array_equal(R.segment_trees(junk, want[0], 0.6, 0.3, 2.0, heights=h)[0], R.segment_trees(pts, want[0], 0.6, 0.3, 2.0)[0])
    # a mask, and non-finite x, y, h
    mask = (np.arange(3000) % 4 != 1).astype(np.uint8)
    bad = pts.copy()
    bad[5::97, 0] = NAN
    bad[11::89, 1] = INF
    bad[13::83, 2] = -INF
    bad[17::79, 2] = NAN
    want, _ = check_tops(hip, bad, VARIABLE, 2.0, mask=mask, what="mask + non-finite")
    check_crowns(hip, bad, want[0], 0.6, 0.3, 2.0, mask=mask, what="mask + non-finite crowns")
    hb = h.copy()
    hb[3::50] = NAN
    check_tops(hip, pts, VARIABLE, 2.0, heights=hb, what="non-finite column")
    # negative heights, and both zeros: they compare equal, so the index decides
    neg = pts.copy()
    neg[:, 2] -= 25.0
    want, _ = check_tops(hip, neg, VARIABLE, -24.0, what="negative")
    check_crowns(hip, neg, want[0], 0.6, 0.3, -24.0, what="negative crowns")
    rng = np.random.default_rng(2)
    zeros = np.column_stack([rng.random((400, 2)) * 20.0, np.where(rng.random(400) < 0.5, 0.0, -0.0)])
    want, _ = check_tops(hip, zeros, (2.0, 0.0, 2.0, 2.0), -1.0, edges=(0.0, 0.5), what="zeros")
    assert want[1].tolist() == sorted(want[1].tolist())  # equal heights: ascending index


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
def test_storages(hip, storage):
    pts = canopy(1500, 31)
    mask = (np.arange(1500) % 5 != 0).astype(np.uint8)
    want, _ = check_tops(hip, pts, VARIABLE, 2.0, mask=mask, storage=storage, what=storage)
    check_crowns(hip, pts, want[0], 0.6, 0.3, 2.0, mask=mask, storage=storage, what=storage)


@pytest.mark.gpu
def test_numbering_and_the_index_capacity(hip):
    pts = np.array([[10.0 * i, 0.0, h] for i, h in enumerate([5, 9, 5, 9, 7, 9, -0.0, 0.0])])
    want, _ = check_tops(hip, pts, (1.0, 0.0, 1.0, 1.0), -1.0, what="ties")
    assert want[1].tolist() == [1, 3, 5, 4, 0, 2, 6, 7]
    nt = len(want[1])
    for cap in (nt, nt + 1):
        top, idx, info = gpu_tops(hip, pts, (1.0, 0.0, 1.0, 1.0), -1.0, capacity=cap)
        assert idx.tolist() == want[1].tolist()
    top, idx, info = gpu_tops(hip, pts, (1.0, 0.0, 1.0, 1.0), -1.0, capacity=-1)  # no list asked for
    assert info["n_tops"] == nt and np.array_equal(top, want[0])
    import torch
    buf = make_buffer(hip, pts, "H")
    topd = torch.zeros(8, dtype=torch.uint8, device="cuda")
    idxd = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    nc, ntops = C.c_uint64(), C.c_uint64()
    with pytest.raises(PastureError) as e:  # too small: the count is reported, the mask written, no list
        hip.tree_tops_device(buf._h, None, None, -1.0, (C.c_double * 4)(1, 0, 1, 1), 0.0, C.c_void_p(topd.data_ptr()), C.c_void_p(idxd.data_ptr()), nt - 1, C.byref(nc),
                             C.byref(ntops), None, None)
    assert e.value.code == 3 and ntops.value == nt and nc.value == 8
    assert topd.cpu().numpy().tolist() == want[0].tolist() and idxd.cpu().numpy().tolist() == [77] * 8
    # the same for the crowns' counts
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    cnt = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    ntr, nl = C.c_uint64(), C.c_uint64()
    with pytest.raises(PastureError) as e:
        hip.segment_trees_device(buf._h, None, None, C.c_void_p(topd.data_ptr()), -1.0, 0.6, 0.3, 0.0, C.c_void_p(ids.data_ptr()), C.c_void_p(cnt.data_ptr()), nt - 1,
                                 C.byref(ntr), C.byref(nl))
    assert e.value.code == 3 and ntr.value == nt and cnt.cpu().numpy().tolist() == [77] * 8
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), R.segment_trees(pts, want[0], 0.6, 0.3, -1.0)[0])


@pytest.mark.gpu
def test_crown_knife_edges_and_parameters(hip):
    # rc = 0.5 * 0.5 * 20 = 5 and exclusion * H = 5: on both edges, one ulp off either, along the axes and on the diagonal
    pts = [[0, 0, 20.0]]
    for dx, dy in ((5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (-4, 3)):
        for beyond in (0, 1):
            ex = np.sign(dx) * up(abs(dx), beyond) if dx else 0.0
            ey = np.sign(dy) * up(abs(dy), beyond) if dy else 0.0
            pts += [[ex, ey, 6.0], [dx, dy, down(5.0, beyond)]]
    pts = np.array(pts)
    tops = np.zeros(len(pts), dtype=np.uint8)
    tops[0] = 1
    want = check_crowns(hip, pts, tops, 0.5, 0.25, 2.0, edges=(0.0, 5.0, 1.0, 1e6), what="knife")
    assert want[0][1:].reshape(-1, 4).tolist() == [[0, 0, NO_TREE, NO_TREE]] * 6  # (the cases are what they claim)
    scene = canopy(4000, 41)
    top = R.tree_tops(scene, VARIABLE, 2.0)[0]
    assert top.sum() >= 6
    for factor, exclusion in ((0.6, 0.0), (0.6, 1.0), (0.0, 0.3), (0.0, 1.0), (5.0, 0.0)):
        want = check_crowns(hip, scene, top, factor, exclusion, 2.0, what=f"factor {factor} exclusion {exclusion}")
        if factor == 0.0 and exclusion == 0.3:
            assert want[2] >= top.sum() and want[1].max() <= 2  # only the tops label themselves (and an exact duplicate, if there is one)
    # a caller-edited mask: a top below min_height, a non-finite one, an ordinary point promoted; then no tops, then one
    edited = top.copy()
    low = int(np.flatnonzero(scene[:, 2] < 1.0)[0])
    edited[low] = 1
    edited[np.flatnonzero(top)[:3]] = 0
    edited[1234] = 1
    holed = scene.copy()
    holed[np.flatnonzero(top)[5], 0] = NAN
    check_crowns(hip, holed, edited, 0.8, 0.2, 2.0, what="edited")
    want = check_crowns(hip, scene, np.zeros(4000, dtype=np.uint8), 0.6, 0.3, 2.0, what="no tops")
    assert (want[0] == NO_TREE).all() and len(want[1]) == 0
    one = np.zeros(4000, dtype=np.uint8)
    one[np.flatnonzero(top)[0]] = 1
    check_crowns(hip, scene, one, 0.6, 0.3, 2.0, edges=(0.0, 1.0), what="one top")


@pytest.mark.gpu
def test_crown_ties_on_the_voronoi_edges(hip):
    """tops on a lattice, every second one lower, queries on the cell edges and corners of the Voronoi diagram: two or four tops at exactly
    the same distance, and the smaller BUFFER index wins whatever its tree number"""
    rng = np.random.default_rng(8)
    gx, gy = np.meshgrid(np.arange(0.0, 40.0, 4.0), np.arange(0.0, 40.0, 4.0))
    tops_xy = np.column_stack([gx.ravel(), gy.ravel()])
    tops = np.column_stack([tops_xy, rng.uniform(10.0, 30.0, len(tops_xy))])[rng.permutation(len(tops_xy))]
    qx, qy = np.meshgrid(np.arange(0.0, 38.0, 2.0), np.arange(0.0, 38.0, 2.0))
    queries = np.column_stack([qx.ravel(), qy.ravel(), np.full(qx.size, 5.0)])
    pts = np.concatenate([queries[:150], tops, queries[150:]])
    mask = np.zeros(len(pts), dtype=np.uint8)
    mask[150:150 + len(tops)] = 1
    want = check_crowns(hip, pts, mask, 0.9, 0.1, 2.0, edges=(0.0, 4.0, 2.0, 1.3, 1e6), what="voronoi")
    assert want[2] > len(tops) + 100


@pytest.mark.gpu
def test_two_calls_write_the_same_bytes(hip):
    pts = canopy(9000, 51)
    a, b = gpu_tops(hip, pts, VARIABLE, 2.0), gpu_tops(hip, pts, VARIABLE, 2.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    c, d = gpu_crowns(hip, pts, a[0], 0.6, 0.3, 2.0), gpu_crowns(hip, pts, a[0], 0.6, 0.3, 2.0)
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes() and c[2] == d[2]


@pytest.mark.gpu
def test_the_scene_of_the_issue(hip):
    pts, trunks, H = stand(20011, 1, 60.0)
    for window in (VARIABLE, (3.0, 0.0, 3.0, 3.0), (0.25, 0.0, 0.25, 0.25)):
        want, _ = check_tops(hip, pts, window, 2.0, what=f"window {window}")
    want = R.tree_tops(pts, VARIABLE, 2.0)
    assert len(want[1]) == len(trunks) == 36
    check_crowns(hip, pts, want[0], 0.6, 0.3, 2.0, what="crowns")
    # the heights from a device column, through the Python layer
    tops = alg.tree_tops(make_buffer(hip, pts, "H"), window=tuple(2.0 * v for v in VARIABLE), min_height=2.0, heights=pts[:, 2].copy())
    assert np.array_equal(tops.indices, want[1]) and np.array_equal(tops.heights, pts[want[1].astype(np.int64), 2]) and tops.n_candidates == want[2]


@pytest.mark.gpu
def test_scale_properties(hip):
    """200 003 points: every top's window holds no dominator, tops == planted trees, every labelled point's tree is its nearest top"""
    pts, trunks, H = stand(200003, 2, 190.0)
    buf = make_buffer(hip, pts, "H")
    tops = alg.tree_tops(buf, window=tuple(2.0 * v for v in VARIABLE), min_height=2.0)
    assert tops.n_tops == len(trunks) == 361
    idx = tops.indices.astype(np.int64)
    assert sorted(map(tuple, pts[idx, :2].tolist())) == sorted(map(tuple, trunks.tolist()))
    assert np.all(np.diff(tops.heights) <= 0.0)
    cand = np.flatnonzero(pts[:, 2] >= 2.0)
    assert tops.n_candidates == len(cand)
    x, y, h = pts[cand, 0], pts[cand, 1], pts[cand, 2]
    r = R.window_radius(pts[idx, 2], VARIABLE)
    d2 = R._d2(pts[idx, 0], pts[idx, 1], x, y)
    dominators = (d2 <= (r * r)[:, None]) & ((h[None, :] > pts[idx, 2][:, None]) | ((h[None, :] == pts[idx, 2][:, None]) & (cand[None, :] < idx[:, None])))
    assert not dominators.any()
    seg = alg.segment_trees(buf, tops, 0.6, 0.3, 2.0)
    assert seg.n_trees == 361 and seg.counts.sum() == seg.n_labelled == (seg.tree_id != NO_TREE).sum()
    sample = np.random.default_rng(9).choice(np.flatnonzero(seg.tree_id != NO_TREE), 2000, replace=False)
    nearest = np.argmin(R._d2(pts[sample, 0], pts[sample, 1], pts[idx, 0], pts[idx, 1]), axis=1)
    assert np.array_equal(seg.tree_id[sample], nearest.astype(np.uint32))
    assert np.array_equal(seg.counts, np.bincount(seg.tree_id[seg.tree_id != NO_TREE].astype(np.int64), minlength=361).astype(np.uint32))


@pytest.mark.gpu
def test_composition(hip):
    pts, trunks, H = stand(20011, 1, 60.0)
    layout = PointLayout.from_attributes([A.POSITION_3D, A.CLASSIFICATION], api=hip)
    buf = HashMapBuffer.new_from_layout(layout)
    buf.resize(len(pts))
    buf.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
    tops = alg.tree_tops(buf, window=tuple(2.0 * v for v in VARIABLE), min_height=2.0)
    seg = alg.segment_trees(buf, tops)
    # extract_tree against filter with a numpy mask: the three tallest trees
    got = alg.extract_tree(buf, seg, first=0, count=3)
    keep = seg.tree_id < 3
    assert got.len() == int(seg.counts[:3].sum()) == int(keep.sum())
    assert np.array_equal(got.view_attribute(A.POSITION_3D), buf.filter(HashMapBuffer, keep).view_attribute(A.POSITION_3D))
    # the labels in device memory
    import torch
    ids = torch.zeros(len(pts), dtype=torch.int32, device="cuda")
    on_device = alg.segment_trees(buf, tops.mask, device_tree_id_ptr=ids.data_ptr())
    assert on_device.tree_id is None and np.array_equal(ids.cpu().numpy().view(np.uint32), seg.tree_id)
    assert np.array_equal(alg.extract_tree(buf, ids.data_ptr(), 0, 3).view_attribute(A.POSITION_3D), got.view_attribute(A.POSITION_3D))
    # pst_buffer_set_u8_from_ids_device accepts the ids: tree t's points get class 100 + t % 50, the others keep theirs
    values = (100 + np.arange(seg.n_trees) % 50).astype(np.uint8)
    vals = dev(values, np.uint8)
    written = C.c_uint64()
    hip.buffer_set_u8_from_ids_device(buf._h, A.CLASSIFICATION.name().encode(), C.c_void_p(ids.data_ptr()), C.c_void_p(vals.data_ptr()), seg.n_trees, C.byref(written))
    torch.cuda.synchronize()
    cls = buf.view_attribute(A.CLASSIFICATION)
    assert written.value == seg.n_labelled
    assert np.array_equal(cls, np.where(seg.tree_id != NO_TREE, values[np.minimum(seg.tree_id, seg.n_trees - 1).astype(np.int64)], 0).astype(np.uint8))


@pytest.mark.gpu
def test_the_example_counts(hip):
    spec = importlib.util.spec_from_file_location("tree_inventory", os.path.join(ROOT, "examples", "tree_inventory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.inventory(n_points=60000, seed=3)
    assert out["planted"] == 36 and out["found"] == out["planted"]
    assert out["n_labelled"] == sum(out["counts"]) and len(out["tallest"]) == 5
    assert out["boxes_found_with_a_small_window"] > 0 and out["tops_on_boxes"] >= 1 and out["dbscan_clusters"] != out["planted"]
