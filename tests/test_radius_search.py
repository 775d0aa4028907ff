"""Fixed-radius neighbour search on the GPU (pst_radius_neighbour_counts_device, pst_radius_search_device) against tests/radius_ref.py.

Every comparison is exact: u32 / u64 / f64-as-u64 views, no tolerance -- sqrt is correctly rounded on both sides.  The sizes sit on the
seams pst_radius_kernel_shape reports: Q queries per workgroup of the count and fill kernels, C the longest list ordered in LDS, W the window
of entries a workgroup sorts, P the entry positions whose lists it owns."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import features_ref as F
import nn_ref
import pasture_amd as pa
import radius_ref as R
from pasture_amd import PastureError
from pasture_amd import algorithms as alg
from test_outliers import make_buffer

pytestmark = pytest.mark.gpu

_S = pa.radius_kernel_shape()
Q, C, W, P = _S["queries_per_block"], _S["sort_cap"], _S["sort_window"], _S["sort_positions_per_block"]
INF = float("inf")
NAN = float("nan")
UTM = np.array([5.0e5, 5.0e6, 100.0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bytes(a, b):
    return (a.offsets.tobytes() == b.offsets.tobytes() and a.indices.tobytes() == b.indices.tobytes() and a.distances.tobytes() == b.distances.tobytes())


def check(got, want, what=""):
    off, idx, dist = want
    assert got.offsets.dtype == np.uint64 and got.indices.dtype == np.uint32 and got.distances.dtype == np.float64, what
    assert np.array_equal(got.offsets, off), f"{what}: offsets differ, first at query {np.flatnonzero(np.diff(got.offsets.astype(np.int64)) != np.diff(off.astype(np.int64)))[:4]}"
    bad = np.flatnonzero((got.indices != idx) | (bits(got.distances) != bits(dist)))
    assert bad.size == 0, f"{what}: {bad.size} of {len(idx)} entries differ, first {bad[:4]}: idx {got.indices[bad[:4]]} vs {idx[bad[:4]]}, dist {got.distances[bad[:4]]} vs {dist[bad[:4]]}"


def run(hip, q, t, radius, transform=None, qs="V", ts="H", cell_edge=0.0):
    """radius_search of q in t through the named storages; the counts call must agree with the lists' offsets"""
    qb, tb = make_buffer(hip, q, qs), make_buffer(hip, t, ts)
    index = alg.NearestNeighbourIndex(tb, cell_edge)
    try:
        got = pa.radius_search(qb, index, radius, transform)
        counts = pa.radius_neighbour_counts(qb, index, radius, transform)
    finally:
        index.destroy()
    assert counts.dtype == np.uint32 and np.array_equal(counts, got.counts)
    return got


def box(n, seed, size=(10.0, 10.0, 10.0)):
    return np.random.default_rng(seed).random((n, 3)) * np.asarray(size)


def clusters(lengths, seed=0, spacing=100.0, spread=1e-3):
    """(queries, targets): query i at (i * spacing, 0, 0) with lengths[i] targets within `spread` of it, in shuffled buffer order"""
    rng = np.random.default_rng(seed)
    q = np.zeros((len(lengths), 3))
    q[:, 0] = np.arange(len(lengths)) * spacing
    t = np.concatenate([q[i] + (rng.random((k, 3)) - 0.5) * spread for i, k in enumerate(lengths)] + [np.zeros((0, 3))])
    return q, t[rng.permutation(len(t))]


# ------------------------------------------------------------------------------------------------------------------- sizes on the seams

@pytest.mark.parametrize("nt", [1, 2, 1000])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, Q - 1, Q, Q + 1, 2 * Q + 1])
def test_query_counts(hip, nq, nt):
    q, t = box(nq, 100 + nq), box(nt, 7)
    radius = 1.3 if nt == 1000 else 6.0
    check(run(hip, q, t, radius), R.search(q, t, radius), f"{nq} x {nt}")


@pytest.mark.parametrize("k", [0, 1, 2, C - 1, C, C + 1, 3 * C + 7])
def test_list_lengths(hip, k):
    """k near-coincident targets around one query, the rest of the cloud far away"""
    q, t = clusters([k, 3, 0, 5, 1])
    got = run(hip, q, t, 0.01)
    assert np.array_equal(got.counts, [k, 3, 0, 5, 1])
    check(got, R.search(q, t, 0.01), f"k = {k}")


@pytest.mark.parametrize("length", [400, C])
@pytest.mark.parametrize("before", [P - 1, P])
def test_list_head_at_the_block_seam(hip, before, length):
    """A list whose head is entry position P - 1 (the last one workgroup 0 owns) or P (the first of workgroup 1).  With `length` = C and the
    head at P - 1 the list ends at position W - 1: it fills the window exactly."""
    first = [C] * (before // C) + [before % C]
    q, t = clusters(first + [length, 7, C, 2, 300, 1])
    got = run(hip, q, t, 0.01)
    assert got.offsets[len(first)] == before and got.counts[len(first)] == length
    check(got, R.search(q, t, 0.01), f"head at {before}, length {length}")


def test_lists_that_fill_windows_exactly(hip):
    """Lists of C entries head to tail over three workgroups' positions: where P + C = W, the list whose head is the last multiple of C
    below P ends at W - 1."""
    q, t = clusters([C] * (3 * P // C) + [1])
    check(run(hip, q, t, 0.01), R.search(q, t, 0.01), "lists of C")


def test_one_list_of_5000(hip):
    q, t = clusters([5000])
    got = run(hip, q, t, 0.01)
    assert got.counts[0] == 5000
    check(got, R.search(q, t, 0.01), "one list of 5000")


@pytest.mark.parametrize("n", [300, C + 150])
def test_all_targets_coincident(hip, n):
    """Every d2 ties: every list is the ascending indices.  n <= C: ordered in LDS; above: by the radix sorts."""
    t = np.tile([[3.0, -2.0, 1.5]], (n, 1))
    got = run(hip, t, t, 0.5, qs="H", ts="H")
    assert np.array_equal(got.counts, np.full(n, n)) and not got.distances.any()
    assert np.array_equal(got.indices.reshape(n, n), np.tile(np.arange(n, dtype=np.uint32), (n, 1)))


# ------------------------------------------------------------------------------------------------------------------- the two ordering paths

def order_path_inputs():
    q, t = clusters([0, 1, 2, 3, 17, C - 1, C, 40, C // 2, 5], seed=4)
    extra = box(600, 11, (900.0, 2.0, 2.0)) + np.array([0.0, 5.0, 0.0])  # (clear of the clusters on y = 0)
    return np.concatenate([q, extra[:50]]), np.concatenate([t, extra])


def _digest(r):
    return hashlib.sha256(r.offsets.tobytes() + r.indices.tobytes() + r.distances.tobytes()).hexdigest()


def child_main():
    """run in a child process whose environment carries PST_RADIUS_SORT_CAP (read once per process): the digest of the lists on stdout"""
    hip = pa.product_api()
    q, t = order_path_inputs()
    print("digest", _digest(run(hip, q, t, 0.6)))


@pytest.mark.parametrize("cap", ["0", "3"])
def test_both_ordering_paths_give_the_same_bytes(hip, cap):
    """The same inputs with every list ordered in LDS (this process: no list is longer than C) and, in a child process, with every list
    (PST_RADIUS_SORT_CAP=0) or every list above 3 entries sent through the radix sorts."""
    q, t = order_path_inputs()
    got = run(hip, q, t, 0.6)
    assert got.counts.max() == C
    check(got, R.search(q, t, 0.6), "in LDS")
    env = dict(os.environ, PST_RADIUS_SORT_CAP=cap)
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_radius_search as T; T.child_main()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"digest {_digest(got)}" in r.stdout


# ------------------------------------------------------------------------------------------------------------------- the knife edge

def lattice(m=5):
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("nudge", [-1, 0, 1])
@pytest.mark.parametrize("r2", [1, 2, 3])
def test_knife_edge_on_the_integer_lattice(hip, r2, nudge):
    pts = lattice()
    radius = math.sqrt(r2)
    radius = np.nextafter(radius, INF) if nudge > 0 else np.nextafter(radius, 0.0) if nudge < 0 else radius
    got = run(hip, pts, pts, radius)
    check(got, R.search(pts, pts, radius), f"r2 = {r2}, nudge {nudge}")
    if nudge > 0:
        assert got.counts[62] == {1: 7, 2: 19, 3: 27}[r2]
    if nudge < 0:
        assert got.counts[62] == {1: 1, 2: 7, 3: 19}[r2]


@pytest.mark.parametrize("nudge", [-1, 0, 1])
@pytest.mark.parametrize("r2", [1, 2, 3])
def test_knife_edge_at_utm_coordinates_with_millimetre_spacing(hip, r2, nudge):
    pts = UTM + lattice() * 0.001
    radius = 0.001 * math.sqrt(r2)
    radius = np.nextafter(radius, INF) if nudge > 0 else np.nextafter(radius, 0.0) if nudge < 0 else radius
    check(run(hip, pts, pts, radius, qs="H"), R.search(pts, pts, radius), f"r2 = {r2}, nudge {nudge}")


# ------------------------------------------------------------------------------------------------------------------- grid independence

def test_the_cell_edge_changes_nothing(hip):
    """The same two clouds with indexes built at an automatic edge, radius / 7.3, radius, 3.1 radius and 100 radius (one cell)."""
    t = np.concatenate([box(3000, 21), box(500, 22, (1.0, 1.0, 1.0)) + 4.0])
    q = np.concatenate([box(700, 23), box(40, 24) * 2.0 - 5.0])
    radius = 0.9
    want = R.search(q, t, radius)
    first = None
    for edge in (0.0, radius / 7.3, radius, 3.1 * radius, 100.0 * radius):
        got = run(hip, q, t, radius, cell_edge=edge)
        check(got, want, f"cell_edge {edge}")
        first = first or got
        assert same_bytes(got, first), edge


# ------------------------------------------------------------------------------------------------------------------- geometry

def test_queries_outside_the_targets_box(hip):
    t = box(2000, 31)
    radius = 1.5
    far = box(50, 32) + np.array([10.0 + 2.0 * radius, 0.0, 0.0])                  # farther than the radius from the box
    near = box(200, 33) * np.array([0.1, 1.0, 1.0]) + np.array([10.0 + 0.2, 0.0, 0.0])  # within it of the x = 10 face
    below = box(100, 34) * np.array([1.0, 1.0, 0.05]) - np.array([0.0, 0.0, 1.0])
    q = np.concatenate([far, near, below])
    got = run(hip, q, t, radius)
    assert not got.counts[:50].any() and got.counts[50:].any()
    check(got, R.search(q, t, radius), "outside")


@pytest.mark.parametrize("shape", ["planar", "collinear", "single", "none_finite"])
def test_degenerate_targets(hip, shape):
    t = box(1500, 41)
    if shape == "planar":
        t[:, 2] = 2.5
    elif shape == "collinear":
        t[:, 1:] = [1.0, -3.0]
    elif shape == "single":
        t = t[:1]
    else:
        t[:, 0] = np.where(np.arange(len(t)) % 2, NAN, INF)
    q = np.concatenate([t[:300], box(100, 42)])
    q[:, 2] += 0.01
    radius = 0.8
    got = run(hip, q, t, radius)
    if shape == "none_finite":
        assert not got.offsets.any() and got.indices.size == 0
    check(got, R.search(q, t, radius), shape)


def test_non_finite_queries_and_targets(hip):
    t, q = box(1200, 51), box(400, 52)
    t[::7, 0] = NAN
    t[3::11, 2] = INF
    t[5::13, 1] = -INF
    q[::5, 1] = NAN
    q[2::9, 0] = INF
    got = run(hip, q, t, 1.4)
    assert not got.counts[::5].any() and not got.counts[2::9].any()
    check(got, R.search(q, t, 1.4), "non-finite")
    # the self-search of the target: a point that is not finite neither finds nor is found
    got = run(hip, t, t, 1.4, qs="H", ts="H")
    check(got, R.search(t, t, 1.4), "self")


def test_transform(hip):
    """A rotation plus translation, against nn_ref.apply_transform; and a transform that overflows some queries to infinity."""
    from test_nearest import rigid
    t = box(2500, 61)
    move = rigid((1.0, 2.0, -1.0), 25.0, (0.3, -0.2, 0.1), about=(5.0, 5.0, 5.0))
    q = box(600, 62)
    want = R.search(q, t, 1.1, move)
    assert np.array_equal(want[0], R.search(nn_ref.apply_transform(q, move), t, 1.1)[0])
    check(run(hip, q, t, 1.1, transform=move), want, "rigid")
    grow = np.array([[1e308, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    q2 = q.copy()
    q2[::2, 0] = 0.0          # these stay at x' = 0, the others overflow to +inf
    got = run(hip, q2, t, 1.1, transform=grow)
    assert not got.counts[1::2].any() and got.counts[::2].any()
    check(got, R.search(q2, t, 1.1, grow), "overflow")


@pytest.mark.parametrize("ts", ["V", "H", "sliceV", "external"])
@pytest.mark.parametrize("qs", ["V", "H", "sliceH", "external", "packedV"])
def test_storages(hip, qs, ts):
    q, t = box(333, 71), box(1111, 72)
    check(run(hip, q, t, 1.2, qs=qs, ts=ts), _storage_reference(), f"{qs} in {ts}")


_CACHE = {}


def _storage_reference():
    if "storage" not in _CACHE:
        _CACHE["storage"] = R.search(box(333, 71), box(1111, 72), 1.2)
    return _CACHE["storage"]


@pytest.mark.parametrize("storage", ["V", "H", "sliceV", "external"])
def test_query_and_target_are_the_same_buffer(hip, storage):
    t = box(900, 73)
    buf = make_buffer(hip, t, storage)
    got = pa.radius_search(buf, buf, 1.3)
    check(got, R.search(t, t, 1.3), storage)
    assert np.array_equal(pa.radius_neighbour_counts(buf, buf, 1.3), got.counts)
    assert np.array_equal(got.indices[got.offsets[:-1].astype(np.int64)], np.arange(900))  # itself first, at distance 0


# ------------------------------------------------------------------------------------------------------------------- capacity

def test_capacity(hip):
    import torch
    q, t = box(500, 81), box(2000, 82)
    radius = 1.2
    off, idx, dist = R.search(q, t, radius)
    total = len(idx)
    qb, tb = make_buffer(hip, q, "V"), make_buffer(hip, t, "H")
    index = alg.NearestNeighbourIndex(tb)
    try:
        d_off = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        d_idx = torch.full((total + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_dist = torch.full((total + 8,), -7.25, dtype=torch.float64, device="cuda")
        # one short: PST_ERR_RANGE, the total in the message, the offsets written, not one byte of the arrays touched
        with pytest.raises(PastureError) as e:
            pa.radius_search_device(qb, index, radius, d_off.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), total - 1)
        assert e.value.code == 3 and f"total = {total}" in str(e.value)
        assert np.array_equal(d_off.cpu().numpy().view(np.uint64), off)
        assert (d_idx.cpu().numpy() == 0x5A5A5A5A).all() and (d_dist.cpu().numpy() == -7.25).all()
        # exactly enough
        d_off.zero_()
        assert pa.radius_search_device(qb, index, radius, d_off.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), total) == total
        got = pa.RadiusNeighbours(d_off.cpu().numpy().view(np.uint64), d_idx.cpu().numpy().view(np.uint32)[:total], d_dist.cpu().numpy()[:total])
        check(got, (off, idx, dist), "capacity = total")
        assert (d_idx.cpu().numpy()[total:] == 0x5A5A5A5A).all() and (d_dist.cpu().numpy()[total:] == -7.25).all()
        # without distances
        d_idx.fill_(0x5A5A5A5A)
        assert pa.radius_search_device(qb, index, radius, d_off.data_ptr(), d_idx.data_ptr(), 0, total + 8) == total
        assert np.array_equal(d_idx.cpu().numpy().view(np.uint32)[:total], idx)
        # the counting form equals radius_neighbour_counts, host and device
        d_off.zero_()
        assert pa.radius_search_device(qb, index, radius, d_off.data_ptr(), 0, 0, 0) == total
        counts = pa.radius_neighbour_counts(qb, index, radius)
        assert np.array_equal(np.diff(d_off.cpu().numpy()), counts.astype(np.int64))
        d_counts = torch.full((len(q) + 2,), 77, dtype=torch.int32, device="cuda")
        assert pa.radius_neighbour_counts(qb, index, radius, device_counts_ptr=d_counts.data_ptr()) == total
        assert np.array_equal(d_counts.cpu().numpy()[:len(q)].view(np.uint32), counts) and (d_counts.cpu().numpy()[len(q):] == 77).all()
        # an empty query: offsets[0] = 0, total 0
        d_off.fill_(9)
        assert pa.radius_search_device(make_buffer(hip, np.zeros((0, 3)), "V"), index, radius, d_off.data_ptr(), d_idx.data_ptr(), 0, 4) == 0
        assert d_off.cpu().numpy()[0] == 0 and d_off.cpu().numpy()[1] == 9
    finally:
        index.destroy()


# ------------------------------------------------------------------------------------------------------------------- determinism

def test_two_calls_give_the_same_bytes_and_a_permutation_maps_through(hip):
    t, q = box(4000, 91), box(900, 92)
    a, b = run(hip, q, t, 1.0), run(hip, q, t, 1.0)
    assert same_bytes(a, b)
    perm = np.random.default_rng(93).permutation(len(t))
    c = run(hip, q, t[perm], 1.0)
    assert np.array_equal(c.offsets, a.offsets)
    rows = np.repeat(np.arange(len(q)), a.counts)
    mapped = perm[c.indices]
    order = np.lexsort((mapped, bits(c.distances), rows))  # the lists as sets of (d2, index): sorted by (distance, mapped index)
    assert np.array_equal(mapped[order], a.indices) and np.array_equal(bits(c.distances[order]), bits(a.distances))


# ------------------------------------------------------------------------------------------------------------------- cross-checks

def sheet(n, seed):
    """A LiDAR-like sheet: about 0.8 points per square metre on gently rolling ground"""
    rng = np.random.default_rng(seed)
    side = math.sqrt(n / 0.8)
    xy = rng.random((n, 2)) * side
    z = 20.0 * np.sin(xy[:, 0] / 40.0) * np.cos(xy[:, 1] / 55.0) + rng.normal(0, 0.05, n)
    return np.column_stack([xy, z])


def _self_search(hip, name):
    """(points, radius, RadiusNeighbours of the self-search), computed once per cloud, at about 8 neighbours"""
    if name not in _CACHE:
        pts, radius = (sheet(200_003, 5), 1.78) if name == "sheet" else (box(100_003, 6, (100.0, 100.0, 10.0)), 1.24)
        got = run(hip, pts, pts, radius, qs="H", ts="H")
        assert 6.0 < got.counts.mean() < 11.0
        for a in (pts, got.offsets, got.indices, got.distances):
            a.setflags(write=False)
        _CACHE[name] = (pts, radius, got)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["sheet", "box"])
def test_counts_equal_the_core_flags_of_dbscan(hip, name):
    """counts >= m is DBSCAN's core flag at eps = radius, min_points = m: the predicate is the same."""
    pts, radius, got = _self_search(hip, name)
    buf = make_buffer(hip, pts, "H")
    for m in (1, 4, 16):
        core = alg.dbscan(buf, radius, m).core
        assert np.array_equal(core, got.counts >= m), m


@pytest.mark.parametrize("name", ["sheet", "box"])
def test_first_entry_equals_nearest_neighbours(hip, name):
    """Queries shifted off the targets: the head of every list and its distance are nearest_neighbours(max_distance = radius); an empty
    list is "no match"."""
    pts, radius, _ = _self_search(hip, name)
    q = pts[::20] + np.array([0.9, -0.7, 0.3]) * radius
    qb, tb = make_buffer(hip, q, "V"), make_buffer(hip, pts, "H")
    index = alg.NearestNeighbourIndex(tb)
    try:
        got = pa.radius_search(qb, index, radius)
        idx, dist = alg.nearest_neighbours(qb, index, radius)
    finally:
        index.destroy()
    empty = got.counts == 0
    assert empty.any() and not empty.all()
    assert np.all(idx[empty] == 0xFFFFFFFF) and np.all(np.isposinf(dist[empty]))
    heads = got.offsets[:-1].astype(np.int64)[~empty]
    assert np.array_equal(got.indices[heads], idx[~empty]) and np.array_equal(bits(got.distances[heads]), bits(dist[~empty]))


def test_brute_force_10007_queries_in_20011_targets(hip):
    t, q = box(20_011, 101, (30.0, 30.0, 30.0)), box(10_007, 102, (30.0, 30.0, 30.0))
    got = run(hip, q, t, 1.37)
    assert 6.0 < got.counts.mean() < 10.0
    check(got, R.search(q, t, 1.37), "10 007 x 20 011")


def test_the_sheet_equals_the_bucketed_grid_reference(hip):
    pts, radius, got = _self_search(hip, "sheet")
    check(got, R.search_grid(pts, pts, radius), "sheet")


def test_padded_lists_feed_geometric_features(hip):
    """to_padded(16) is what geometric_features(knn=...) takes: features over radius neighbourhoods, equal to the restatement's features of
    the same padded lists."""
    pts = sheet(5000, 7)
    buf = make_buffer(hip, pts, "H")
    got = pa.radius_search(buf, buf, 2.5)
    knn = got.to_padded(16)
    assert knn.shape == (5000, 16) and (knn == 0xFFFFFFFF).any() and (got.counts > 16).any()
    names = ("linearity", "planarity", "scattering", "verticality", "count")
    r = alg.geometric_features(buf, 16, features=names, knn=knn)
    ref = F.features(pts, knn)
    assert np.array_equal(r["count"], np.minimum(got.counts, 16).astype(np.float64))
    for name in names:
        assert np.array_equal(bits(r[name]), bits(ref[name])), name


def test_more_than_2_32_entries_are_refused_after_the_count(hip):
    """65 536 coincident points: 2^32 entries.  PST_ERR_UNSUPPORTED with the offsets and the total written, and the counts call still works."""
    import torch
    t = np.tile([[1.0, 2.0, 3.0]], (65_536, 1))
    buf = make_buffer(hip, t, "H")
    index = alg.NearestNeighbourIndex(buf)
    try:
        d_off = torch.zeros(len(t) + 1, dtype=torch.int64, device="cuda")
        total = len(t) * len(t)
        assert total >= 0xFFFFFFF0
        d_idx = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # (never written: the refusal comes before the fill)
        with pytest.raises(PastureError) as e:
            pa.radius_search_device(buf, index, 0.5, d_off.data_ptr(), d_idx.data_ptr(), 0, total)
        assert e.value.code == 23 and (d_idx.cpu().numpy() == 0x5A5A5A5A).all()
        assert d_off.cpu().numpy()[-1] == total and d_off.cpu().numpy()[1] == len(t)
        assert pa.radius_neighbour_counts(buf, index, 0.5, device_counts_ptr=None)[0] == len(t)
    finally:
        index.destroy()
