"""Segment statistics (pst_segment_statistics, pst_segments_kernel_shape, pst_segments_phase_times) against tests/segments_ref.py.

CPU tests pin the restatement on a hand-computed table, the tree of its sums, and the argument checks answered on the host.  GPU tests
compare the HIP path with the restatement BIT FOR BIT (u64 views: NaNs as bits, -0.0 apart from +0.0), no tolerance anywhere: counts, boxes,
extremes and the apex do not depend on any order, the sums have the fixed tree of the header, and numpy's float64 arithmetic rounds every
operation once, as the kernels do."""
import ctypes as C

import numpy as np
import pytest

import raster_ref as R
import segments_ref as G
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from test_outliers import make_buffer

POINTS_PER_BLOCK = 256  # asserted against pst_segments_kernel_shape below: the parametrisations need them at collection time
GROUP = 256
GROUPS_PER_BLOCK = 4
ALL = G.STATS
ORDER_FREE = ("count", "bounds", "value_min", "value_max")
SEEDS = (1, 10)  # two, because one seed's tree and plain sums agree at some lengths (test_the_tree_shows_its_order_at_every_tested_length)
NONE = 0xFFFFFFFF
SEAM_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 191, 192, 193, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 65536 + 256 + 1]
FOUR_LEVELS = (1 << 24) + 1


def _code(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _empty_buffer(hip, dtype=T.Vec3f64, kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(dtype)], api=hip))


def cloud(n, seed):
    """n points whose three coordinates each span 30 decades with mixed signs, so that every sum shows the order of its additions"""
    return np.column_stack([R.wide_values(n, seed), R.wide_values(n, seed + 100), R.wide_values(n, seed + 200)])


def _dev(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size == 0:
        a = np.zeros(1, dtype=dtype)  # (an address that is not NULL; nothing of it is read)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).cuda()


def gpu_stats(hip, pts, labels, S, stats=ALL, values=None, mask=None, storage="H", device_out=False, buf=None, apex=True):
    """-> (planes [P][S] as pst_segment_statistics wrote them, apex or None, n_members), through the C ABI; labels, values and mask go
    through device memory; device results are written between guard entries, which must stay as they were"""
    import torch
    buf = buf if buf is not None else make_buffer(hip, np.asarray(pts, dtype=np.float64).reshape(-1, 3), storage)
    dl = _dev((np.asarray(labels).astype(np.int64) & NONE).astype(np.uint32), np.uint32)
    dv = _dev(values, np.float64) if values is not None else None
    dm = _dev(mask, np.uint8) if mask is not None else None
    word, P = sum(G.BITS[s] for s in stats), sum(G.PLANES[s] for s in stats)
    members = C.c_uint64(99)
    args = (buf._h, C.c_void_p(dl.data_ptr()), S, C.c_void_p(dv.data_ptr()) if dv is not None else None, C.c_void_p(dm.data_ptr()) if dm is not None else None, word)
    if device_out:
        d = torch.full((P * S + 2,), 123.0, dtype=torch.float64, device="cuda")
        a = torch.full((S + 2,), 77, dtype=torch.int32, device="cuda")
        hip.segment_statistics(*args, C.c_void_p(d.data_ptr() + 8), C.c_void_p(a.data_ptr() + 4) if apex else None, 0, C.byref(members))
        d, a = d.cpu().numpy(), a.cpu().numpy().view(np.uint32)
        assert d[0] == 123.0 and d[-1] == 123.0 and a[0] == 77 and a[-1] == 77, "a guard entry around the device results was written"
        if not apex:
            assert (a == 77).all()
        return d[1:-1].reshape(P, S), a[1:-1].copy() if apex else None, members.value
    out = np.full((P, S), 5.0)
    ap = np.full(S, 7, dtype=np.uint32)
    hip.segment_statistics(*args, C.c_void_p(out.ctypes.data), C.c_void_p(ap.ctypes.data) if apex else None, 1, C.byref(members))
    return out, ap if apex else None, members.value


def assert_same(got, want, stats, what=""):
    got_planes, got_apex, got_members = got
    want_planes = G.planes(want[0], stats)
    assert got_planes.shape == want_planes.shape, (what, got_planes.shape, want_planes.shape)
    bad = np.argwhere(G.bits(got_planes) != G.bits(want_planes))
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first (plane, segment) {bad[:3].tolist()}: {got_planes[tuple(bad[0])]!r} vs {want_planes[tuple(bad[0])]!r}"
    if got_apex is not None:
        bad = np.flatnonzero(got_apex != want[1])
        assert bad.size == 0, f"{what}: the apex of {len(bad)} segments differs, first {bad[:3].tolist()}: {got_apex[bad[:3]]} vs {want[1][bad[:3]]}"
    assert got_members == want[2], (what, got_members, want[2])


def check(hip, pts, labels, S, stats=ALL, what="", **kw):
    want = G.statistics(pts, labels, S, stats, values=kw.get("values"), mask=kw.get("mask"))
    got = gpu_stats(hip, pts, labels, S, stats, **kw)
    assert_same(got, want, stats, what)
    return got


# ------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_restatement_on_a_hand_computed_table():
    """Three segments.  0 holds (1, 2, 3) and (3, 4, 5); 1 is empty; 2 holds a -0.0 / +0.0 pair in z.  A label >= S, a 0xFFFFFFFF, a NaN z,
    an infinite x and a masked-out point are no members."""
    inf, nan = np.inf, np.nan
    pts = np.array([[3.0, 4.0, 5.0], [0.0, 0.0, -0.0], [9.0, 9.0, 9.0], [1.0, 2.0, 3.0], [8.0, 8.0, 8.0], [0.0, 0.0, 0.0], [1.0, 1.0, nan], [inf, 1.0, 1.0],
                    [100.0, 100.0, 100.0]])
    labels = np.array([0, 2, 3, 0, NONE, 2, 0, 0, 0])
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)
    got, apex, members = G.statistics(pts, labels, 3, mask=mask)
    n = G.NAN
    assert members == 4 and apex.tolist() == [0, NONE, 5]
    expect = {"count": [[2.0, 0.0, 2.0]],
              "bounds": [[1.0, n, 0.0], [2.0, n, 0.0], [3.0, n, -0.0], [3.0, n, 0.0], [4.0, n, 0.0], [5.0, n, 0.0]],
              "centroid": [[2.0, n, 0.0], [3.0, n, 0.0], [4.0, n, 0.0]],
              "covariance": [[1.0, n, 0.0]] * 6,
              "value_min": [[3.0, n, -0.0]], "value_max": [[5.0, n, 0.0]], "value_mean": [[4.0, n, 0.0]], "value_variance": [[1.0, n, 0.0]]}
    for s in ALL:
        assert np.array_equal(G.bits(got[s]), G.bits(np.array(expect[s]))), (s, got[s])
    assert G.bits(got["bounds"])[2, 2] == 0x8000000000000000 and G.bits(got["bounds"])[5, 2] == 0  # -0.0 is below +0.0, and both keep their bits
    assert (G.bits(got["centroid"])[0, 1], G.bits(got["count"])[0, 1]) == (0x7FF8000000000000, 0)  # an empty segment: the canonical NaN, count +0.0
    # the other order of the pair: the same extremes, and the apex of a tie is the LOWEST index of the largest bits
    again, apex_again, _ = G.statistics(pts[::-1], labels[::-1], 3, mask=mask[::-1])
    for s in ORDER_FREE:
        assert np.array_equal(G.bits(again[s]), G.bits(got[s])), s
    assert apex_again.tolist() == [8, NONE, 3]
    tie = G.statistics(np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 7.0], [0.0, 0.0, 7.0]]), [0, 0, 0], 1)[1]
    assert tie.tolist() == [1]
    # values instead of z: z takes no part in the statistics of the value, but stays a coordinate
    by_value = G.statistics(pts[:6], labels[:6], 3, values=np.array([1.0, 2.0, 3.0, nan, 5.0, 6.0]))
    assert by_value[2] == 3 and by_value[0]["count"][0].tolist() == [1.0, 0.0, 2.0] and by_value[0]["value_mean"][0].tolist()[::2] == [1.0, 4.0]
    assert G.planes(got, ("centroid", "count")).shape == (4, 3) and G.planes(got, ("centroid", "count"))[0].tolist() == [2.0, 0.0, 2.0]  # ascending bit order


def test_the_tree_of_the_sums():
    v = R.wide_values(GROUP + 1, SEEDS[0])
    with np.errstate(all="ignore"):
        r = ((v[0:64] + v[64:128]) + v[128:192]) + v[192:256]
        for h in (32, 16, 8, 4, 2, 1):
            r = r[:h] + r[h:2 * h]
        by_hand = r[0] + v[GROUP]  # the second group is one element: itself; the second level is one group of two
    assert G.bits(G.tree_sum(v)) == G.bits(by_hand)
    assert G.bits(G.tree_sum(v[:GROUP])) == G.bits(r[0])
    # -0.0 is the identity: a lone element is itself, signs of zero included, and one level more changes nothing
    minus, plus = G.bits(np.float64(-0.0)), G.bits(np.float64(0.0))
    assert G.bits(G.tree_sum([-0.0])) == minus and G.bits(G.tree_level([-0.0])[0]) == minus and G.bits(G.tree_level(G.tree_level([-0.0]))[0]) == minus
    assert G.bits(G.tree_sum([0.0])) == plus and G.bits(G.tree_level([0.0])[0]) == plus
    assert G.bits(G.tree_sum([-0.0, -0.0])) == minus and G.bits(G.tree_sum([-0.0, 0.0])) == plus
    for m in (1, 2, 63, GROUP, GROUP + 1):
        w = R.wide_values(m, 3)
        assert G.bits(G.tree_level(np.array([G.tree_sum(w)]))[0]) == G.bits(G.tree_sum(w))
    # the depth: 2 levels up to 65 536, 3 up to 2^24, 4 beyond
    for m, levels in ((GROUP, 1), (GROUP + 1, 2), (65536, 2), (65537, 3)):
        w, k = np.ones(m), 0
        while len(w) > 1:
            w, k = G.tree_level(w), k + 1
        assert k == levels and w[0] == m


def test_the_tree_shows_its_order_at_every_tested_length():
    """A GPU test on these values could not see a wrong order of additions at a length at which the tree and the plain left-to-right sum
    agree in every bit for every seed in use: at every tested length above 2 at least one seed must tell them apart."""
    for m in SEAM_LENGTHS:
        if m <= 2:
            continue
        differs = []
        for seed in SEEDS:
            x = cloud(m, seed)[:, 0]
            differs.append(G.bits(G.tree_sum(x)) != G.bits(np.cumsum(x)[-1]))  # (cumsum adds left to right, one rounding each)
        assert any(differs), m
    z = R.wide_values(200003, 7)
    assert G.bits(np.cumsum(z)[-1]) == G.bits(R.plain_sum(z))
    assert G.bits(G.tree_sum(z)) != G.bits(R.plain_sum(z)) and G.bits(G.tree_sum(z)) != G.bits(R.chunked_sum(z))


def test_the_tree_folds_sixteen_million_values_quickly():
    import time
    v = np.ones(FOUR_LEVELS)
    t0 = time.perf_counter()
    assert G.tree_sum(v) == FOUR_LEVELS
    assert time.perf_counter() - t0 < 1.0


def test_kernel_shape(hip):
    assert alg.segments_kernel_shape(hip) == {"points_per_block": POINTS_PER_BLOCK, "group": GROUP, "groups_per_block": GROUPS_PER_BLOCK}
    assert G.GROUP == GROUP
    one = C.c_uint32(7)
    hip.segments_kernel_shape(None, None, C.byref(one))  # each pointer is optional
    assert one.value == GROUPS_PER_BLOCK
    hip.segments_kernel_shape(None, None, None)
    assert alg.segments_phase_times(hip) == (0.0, 0.0, 0.0)
    assert _code(lambda: hip.segments_phase_times(None)) == 1


def test_argument_errors_answered_on_the_host(hip):
    """Null arguments, invalid parameters and a missing position: the same answer with or without a device, because none is looked for --
    and in that order."""
    buf = _empty_buffer(hip)
    out, apex, members = (C.c_double * 32)(*([5.0] * 32)), (C.c_uint32 * 2)(7, 7), C.c_uint64(9)
    labels = C.c_void_p(8)  # (never read: every call below is refused first)

    def call(b=buf._h, lab=labels, S=2, stats=1, dst=out, kind=1, m=C.byref(members)):
        return lambda: hip.segment_statistics(b, lab, S, None, None, stats, dst, apex, kind, m)
    assert _code(call(b=None)) == 1 and _code(call(lab=None)) == 1 and _code(call(dst=None)) == 1 and _code(call(m=None)) == 1
    assert _code(call(kind=7)) == 1  # no such memory kind
    for stats in (0, 256, 257, 1 << 31):
        assert _code(call(stats=stats)) == 1, stats
    assert _code(call(S=0)) == 1
    # a position that is not Vec3f64 is known from the layout alone -- and is looked at AFTER the parameters
    f32 = _empty_buffer(hip, T.Vec3f32)
    assert _code(call(b=f32._h)) == 4 and _code(call(b=f32._h, S=0)) == 1 and _code(call(b=f32._h, stats=0)) == 1 and _code(call(b=f32._h, lab=None)) == 1
    with pytest.raises(PasturePanic):
        call(b=f32._h)()
    assert list(out) == [5.0] * 32 and list(apex) == [7, 7]  # nothing was written
    with pytest.raises(ValueError):
        alg.segment_statistics(buf, np.zeros(0, dtype=np.uint32), 2, ("median",))
    with pytest.raises(ValueError):
        alg.segment_statistics(buf, np.zeros(3, dtype=np.uint32), 2)  # three labels for no points
    assert alg.segment_stats_bits(ALL) == 255 and alg.segment_planes(255) == 20 and alg.segment_stats_bits("bounds") == 2
    assert [alg.SEGMENT_STATS[s] for s in ALL] == [(G.BITS[s], G.PLANES[s]) for s in ALL]


def test_no_device_is_an_error_not_a_cpu_path(hip):
    import torch
    if torch.cuda.is_available():
        return  # (with a device these calls are the GPU tests below)
    buf = _empty_buffer(hip)
    out, members = (C.c_double * 4)(), C.c_uint64()
    assert _code(lambda: hip.segment_statistics(buf._h, C.c_void_p(8), 2, None, None, 1, out, None, 1, C.byref(members))) == 21
    assert _code(lambda: hip.segment_statistics(buf._h, C.c_void_p(8), (1 << 28) + 1, None, None, 1, out, None, 1, C.byref(members))) == 21  # the device comes first


def test_principal_axes_on_the_host():
    cov = np.array([np.diag([4.0, 1.0, 0.25]), np.full((3, 3), np.nan)])
    table = alg.SegmentTable(2, 5, covariance=cov)
    values, vectors = table.principal_axes()
    assert values[0].tolist() == [0.25, 1.0, 4.0] and np.isnan(values[1]).all() and np.isnan(vectors[1]).all()
    assert np.allclose(np.abs(vectors[0][:, 2]), [1.0, 0.0, 0.0])  # the main direction: x
    with pytest.raises(ValueError):
        alg.SegmentTable(2, 5).principal_axes()


# ------------------------------------------------------------------------------------------------------------------------------ GPU

def _one_segment(m, seed, neighbours):
    """(pts, labels, S): a segment of m members alone, or between neighbours of 1 and 300 members with the labels shuffled over the buffer"""
    if not neighbours:
        return cloud(m, seed), np.zeros(m, dtype=np.uint32), 1
    labels = np.concatenate([np.zeros(1), np.ones(m), np.full(300, 2)]).astype(np.uint32)
    np.random.default_rng(seed + 50).shuffle(labels)
    return cloud(len(labels), seed), labels, 3


@pytest.mark.gpu
@pytest.mark.parametrize("neighbours", [False, True], ids=["alone", "between"])
@pytest.mark.parametrize("m", SEAM_LENGTHS)
def test_segment_length_seams(hip, m, neighbours):
    for seed in SEEDS:
        pts, labels, S = _one_segment(m, seed, neighbours)
        check(hip, pts, labels, S, what=f"m {m} seed {seed}")


@pytest.mark.gpu
def test_the_fourth_level(hip):
    """2^24 + 1 members of one segment: 65 537 groups, 257 partials of partials, 2 of those, one value"""
    w = R.wide_values(FOUR_LEVELS, SEEDS[0])
    pts = np.column_stack([w, w[::-1], np.roll(w, 12345)])
    labels = np.zeros(FOUR_LEVELS, dtype=np.uint32)
    check(hip, pts, labels, 1, what="2^24 + 1")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, 3 * POINTS_PER_BLOCK + 5])
def test_point_count_seams(hip, n):
    rng = np.random.default_rng(n)
    labels = rng.integers(0, 4, n).astype(np.uint32)  # label 3 is no segment of S = 3
    check(hip, cloud(n, 2), labels, 3, what=f"n {n}")
    check(hip, cloud(n, 3), np.zeros(n, dtype=np.uint32), 1, what=f"n {n}, one segment")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 65535, 65536, 65537, 1 << 20])
def test_segment_count_seams(hip, S):
    """around the sort's key widths and pass counts; empty segments at the front, in the middle and at the end"""
    n = 1000
    rng = np.random.default_rng(S)
    labels = rng.integers(0, S, n).astype(np.uint32)
    if S > 8:
        labels[(labels == 0) | (labels == S // 2) | (labels == S - 1)] = 1
        labels[:3] = [S - 2, 2, S // 2 + 1]
    got = check(hip, cloud(n, 4), labels, S, what=f"S {S}")
    if S > 8:
        assert got[0][0, [0, S // 2, S - 1]].tolist() == [0.0, 0.0, 0.0] and got[1][[0, S // 2, S - 1]].tolist() == [NONE] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
def test_no_members_at_all(hip, device_out):
    pts = cloud(700, 5)
    for what, labels in (("every label absent", np.full(700, NONE)), ("every label too large", np.full(700, 5))):
        planes, apex, members = check(hip, pts, labels, 5, what=what, device_out=device_out)
        assert members == 0 and (apex == NONE).all() and (planes[0] == 0.0).all() and (G.bits(planes[1:]) == G.NAN_BITS).all()
    # an empty buffer is legal: every segment is empty
    for kind in (HashMapBuffer, VectorBuffer):
        got = gpu_stats(hip, np.zeros((0, 3)), np.zeros(0), 4, buf=_empty_buffer(hip, kind=kind), device_out=device_out)
        assert_same(got, G.statistics(np.zeros((0, 3)), np.zeros(0), 4), ALL, "empty buffer")
    table = alg.segment_statistics(_empty_buffer(hip), np.zeros(0, dtype=np.uint32), 2, return_apex=True)
    assert table.n_members == 0 and table.count.tolist() == [0.0, 0.0] and table.apex.tolist() == [NONE, NONE] and np.isnan(table.centroid).all()


@pytest.mark.gpu
def test_exactly_one_point_without_a_segment(hip):
    """1 025 points in 3 segments and one of them in none, wherever it stands in the buffer: the only non-member is the last sorted entry,
    the first lane of a workgroup of its own in the directory's heads kernel, and the member count is its sorted position"""
    n = 4 * POINTS_PER_BLOCK + 1
    for at in (0, n // 2, n - 1):
        labels = (np.arange(n) % 3).astype(np.uint32)
        labels[at] = NONE
        got = check(hip, cloud(n, 9), labels, 3, what=f"the point without a segment at {at}")
        assert got[2] == n - 1 and got[0][0].sum() == n - 1


@pytest.mark.gpu
def test_small_segments(hip):
    """5 000 segments of 1 .. 40 members, shuffled: the regime of the regions"""
    rng = np.random.default_rng(6)
    sizes = rng.integers(1, 41, 5000)
    labels = np.repeat(np.arange(5000), sizes).astype(np.uint32)
    rng.shuffle(labels)
    check(hip, cloud(len(labels), 6), labels, 5000, what="small segments")


@pytest.mark.gpu
def test_members(hip):
    n, S = 3000, 4
    rng = np.random.default_rng(7)
    pts = cloud(n, 7)
    labels = rng.integers(0, 6, n).astype(np.uint32)  # 4 and 5: labels >= S
    labels[rng.random(n) < 0.1] = NONE
    for c, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (0, -np.inf), (2, np.nan)):
        pts[rng.integers(0, n, 40), c] = bad
    values = R.wide_values(n, 8)
    values[rng.integers(0, n, 60)] = np.nan
    values[rng.integers(0, n, 60)] = np.inf
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask[mask != 0] = rng.integers(1, 256, int(mask.sum()))  # any non-zero byte
    with_z = check(hip, pts, labels, S, what="z")
    with_values = check(hip, pts, labels, S, values=values, what="values")
    check(hip, pts, labels, S, mask=mask, what="mask")
    check(hip, pts, labels, S, values=values, mask=mask, what="values and mask")
    assert with_values[2] < with_z[2]  # a value that is not finite takes its point out, whatever its z


@pytest.mark.gpu
def test_zeros_and_their_signs(hip):
    z = np.array([-0.0, 0.0, 0.0, -0.0, -0.0])
    pts = np.column_stack([z, z[::-1], z])
    planes, apex, _ = check(hip, pts, [0, 0, 1, 1, 2], 3, what="zeros")
    names = [s for s in ALL for _ in range(G.PLANES[s])]
    centroid_z, vmin, vmax = names.index("centroid") + 2, names.index("value_min"), names.index("value_max")
    minus, plus = 0x8000000000000000, 0
    assert G.bits(planes)[centroid_z].tolist() == [plus, plus, minus]  # a single -0.0 member keeps its sign in the centroid
    assert G.bits(planes)[vmin].tolist() == [minus, minus, minus] and G.bits(planes)[vmax].tolist() == [plus, plus, minus]
    assert apex.tolist() == [1, 2, 4]  # the lowest index among the members with the BITS of the largest value


@pytest.mark.gpu
def test_apex_ties_go_to_the_lowest_index(hip):
    """few different values over 70 001 members: the largest one appears in every group and at every level"""
    m = 70001
    rng = np.random.default_rng(9)
    pts = cloud(m + 500, 9)
    pts[:, 2] = rng.integers(0, 5, m + 500).astype(np.float64)
    labels = np.concatenate([np.zeros(m), np.ones(500)]).astype(np.uint32)
    rng.shuffle(labels)
    _, apex, _ = check(hip, pts, labels, 2, what="ties")
    for s in (0, 1):
        assert apex[s] == np.flatnonzero((labels == s) & (pts[:, 2] == 4.0))[0]
    # the largest value only at the very end, and only at the start, of a segment of three levels
    for at in (m - 1, 0, 65536):
        z = np.zeros(m)
        z[at] = 1.0
        pts = np.column_stack([z, z, z])
        _, apex, _ = check(hip, pts, np.zeros(m, dtype=np.uint32), 1, stats=("value_max",), what=f"largest at {at}")
        assert apex[0] == at


@pytest.mark.gpu
def test_cancellation_at_utm_offsets(hip):
    """extents of metres at offsets of millions: the two-pass covariance, bit for bit"""
    rng = np.random.default_rng(11)
    n = 20000
    pts = np.column_stack([4.0e6 + rng.normal(0.0, 3.0, n), 5.0e5 + rng.normal(0.0, 2.0, n), 300.0 + rng.normal(0.0, 1.0, n)])
    labels = rng.integers(0, 7, n).astype(np.uint32)
    labels[:9000] = 3  # and one large object
    planes, _, _ = check(hip, pts, labels, 7, what="utm")
    names = [s for s in ALL for _ in range(G.PLANES[s])]
    xx = planes[names.index("covariance")]
    assert (np.abs(xx - 9.0) < 1.0).all()  # (the numbers mean something: the variance of x is about 3^2)


@pytest.mark.gpu
@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
def test_every_statistic_alone_and_all_of_them(hip, device_out):
    n, S = 2000, 5
    pts = cloud(n, 12)
    labels = np.random.default_rng(12).integers(0, S + 1, n).astype(np.uint32)
    values = R.wide_values(n, 13)
    buf = make_buffer(hip, pts, "H")
    want = G.statistics(pts, labels, S, ALL, values=values)
    for stats in [(s,) for s in ALL] + [ALL, ("covariance", "count"), ("value_variance", "bounds"), ("centroid", "value_max")]:
        for apex in (True, False):
            got = gpu_stats(hip, pts, labels, S, stats, values=values, buf=buf, device_out=device_out, apex=apex)
            assert_same(got, ({s: want[0][s] for s in stats}, want[1], want[2]), stats, f"{stats} apex {apex}")
    # the plane order is the bit order, whatever the order of the names
    a = gpu_stats(hip, pts, labels, S, ("value_mean", "count"), values=values, buf=buf)[0]
    assert np.array_equal(G.bits(a), G.bits(np.concatenate([want[0]["count"], want[0]["value_mean"]])))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["H", "V", "packedH", "packedV", "sliceH", "slicepackedV", "external"])
def test_storages(hip, storage):
    n, S = 1500, 6
    pts = cloud(n, 14)
    labels = np.random.default_rng(14).integers(0, S, n).astype(np.uint32)
    check(hip, pts, labels, S, storage=storage, what=storage)


@pytest.mark.gpu
def test_determinism_and_permutation(hip):
    n, S = 100000, 50
    rng = np.random.default_rng(15)
    pts = cloud(n, 15)
    labels = rng.integers(0, S, n).astype(np.uint32)
    labels[rng.random(n) < 0.6] = 7  # one segment with most of the points
    buf = make_buffer(hip, pts, "H")
    first = check(hip, pts, labels, S, buf=buf, what="first")
    again = gpu_stats(hip, pts, labels, S, buf=buf)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    perm = rng.permutation(n)
    permuted = check(hip, pts[perm], labels[perm], S, what="permuted")  # the sums: the restatement of the permuted order
    names = [s for s in ALL for _ in range(G.PLANES[s])]
    free = [i for i, s in enumerate(names) if s in ORDER_FREE]
    assert np.array_equal(G.bits(permuted[0][free]), G.bits(first[0][free]))
    assert np.array_equal(perm[permuted[1]], first[1])  # no ties among these values: the same point is the apex


@pytest.mark.gpu
def test_python_table(hip):
    n, S = 4000, 4
    pts = cloud(n, 16)
    labels = np.random.default_rng(16).integers(-1, S, n)  # -1: no segment
    want, apex, members = G.statistics(pts, labels, S)
    buf = make_buffer(hip, pts, "V")
    t = alg.segment_statistics(buf, labels, S, ALL, return_apex=True)
    assert (t.n_segments, t.n_members) == (S, members) and np.array_equal(t.apex, apex)
    assert np.array_equal(G.bits(t.count), G.bits(want["count"][0]))
    assert np.array_equal(G.bits(t.min), G.bits(want["bounds"][:3].T)) and np.array_equal(G.bits(t.max), G.bits(want["bounds"][3:].T))
    assert np.array_equal(G.bits(t.centroid), G.bits(want["centroid"].T))
    xx, xy, xz, yy, yz, zz = want["covariance"]
    assert t.covariance.shape == (S, 3, 3)
    assert np.array_equal(G.bits(t.covariance), G.bits(np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]).transpose(2, 0, 1)))
    for s in ("value_min", "value_max", "value_mean", "value_variance"):
        assert np.array_equal(G.bits(getattr(t, s)), G.bits(want[s][0])), s
    default = alg.segment_statistics(buf, labels, S)
    assert default.covariance is None and default.apex is None and default.value_max is None and np.array_equal(G.bits(default.centroid), G.bits(t.centroid))
    values, vectors = t.principal_axes()
    assert values.shape == (S, 3) and vectors.shape == (S, 3, 3) and (np.diff(values, axis=1) >= 0).all()
    # device labels and device results
    import torch
    dl = _dev((labels.astype(np.int64) & NONE).astype(np.uint32), np.uint32)
    d = torch.zeros((alg.segment_planes(255), S), dtype=torch.float64, device="cuda")
    a = torch.zeros(S, dtype=torch.int32, device="cuda")
    on_device = alg.segment_statistics(buf, dl.data_ptr(), S, ALL, device_out_ptr=d.data_ptr(), device_apex_ptr=a.data_ptr())
    assert on_device.count is None and on_device.n_members == members
    assert np.array_equal(G.bits(d.cpu().numpy()), G.bits(G.planes(want, ALL))) and np.array_equal(a.cpu().numpy().view(np.uint32), apex)


@pytest.fixture(scope="module")
def blobs(hip):
    """200 003 points in 40 dense blobs, in a columnar buffer"""
    n = 200003
    rng = np.random.default_rng(17)
    centres = rng.uniform(0.0, 100.0, (40, 3))
    pts = centres[rng.integers(0, 40, n)] + rng.normal(0.0, 0.3, (n, 3))
    return pts, make_buffer(hip, pts, "H")


@pytest.mark.gpu
def test_against_the_clusterings_of_the_library(hip, blobs):
    pts, buf = blobs
    labels, sizes = alg.euclidean_clusters(buf, 0.25)
    t = alg.segment_statistics(buf, labels, len(sizes), ("count", "bounds"))
    assert np.array_equal(t.count, sizes.astype(np.float64)) and t.n_members == int(sizes.sum())
    for c in range(3):  # the three largest: the box of the compacted cluster, bit for bit
        box = alg.calculate_bounds(alg.extract_clusters(buf, 0.25, first_cluster=c)[0])
        assert G.bits(np.array(box.min())).tolist() == G.bits(t.min[c]).tolist() and G.bits(np.array(box.max())).tolist() == G.bits(t.max[c]).tolist()
    r = alg.dbscan(buf, 0.25, 8)
    t = alg.segment_statistics(buf, r.labels, len(r.sizes), ("count",))
    assert np.array_equal(t.count, r.sizes.astype(np.float64)) and t.n_members == r.n_labelled


@pytest.mark.gpu
def test_the_apex_of_every_tree(hip):
    """a canopy of 200 003 points over 60 crowns: the apex of every tree of segment_trees is one of its points, with its largest height"""
    n = 200003
    rng = np.random.default_rng(18)
    xy = rng.uniform(0.0, 120.0, (n, 2))
    tops = rng.uniform(5.0, 115.0, (60, 2))
    height = rng.uniform(8.0, 25.0, 60)
    d2 = ((xy[:, None, :] - tops[None, :, :]) ** 2).sum(axis=2)
    heights = np.maximum((height[None, :] * np.exp(-d2 / 18.0)).max(axis=1), 0.0) + rng.uniform(0.0, 0.05, n)
    pts = np.column_stack([xy, np.full(n, 100.0)])
    buf = make_buffer(hip, pts, "H")
    seg = alg.segment_trees(buf, alg.tree_tops(buf, 4.0, 2.0, heights=heights), heights=heights)
    assert seg.n_trees > 20
    t = alg.segment_statistics(buf, seg.tree_id, seg.n_trees, ("count", "value_max"), values=heights, return_apex=True)
    assert np.array_equal(t.count, seg.counts.astype(np.float64))
    for tree in range(seg.n_trees):
        if seg.counts[tree] == 0:
            assert t.apex[tree] == NONE
            continue
        own = np.flatnonzero(seg.tree_id == tree)
        assert seg.tree_id[t.apex[tree]] == tree and heights[t.apex[tree]] == heights[own].max() == t.value_max[tree]
        assert t.apex[tree] == own[np.argmax(heights[own])]


@pytest.mark.gpu
def test_refusals_that_need_the_device(hip):
    pts = cloud(10, 19)
    buf = make_buffer(hip, pts, "H")
    labels = _dev(np.zeros(10, dtype=np.uint32), np.uint32)
    out, members = (C.c_double * 4)(*([5.0] * 4)), C.c_uint64()

    def call(b, S):
        return lambda: hip.segment_statistics(b._h, C.c_void_p(labels.data_ptr()), S, None, None, 1, out, None, 1, C.byref(members))
    assert _code(call(buf, (1 << 28) + 1)) == 23 and _code(call(buf, NONE)) == 23
    f32 = VectorBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D.with_custom_datatype(T.Vec3f32)], api=hip))
    f32.resize(10)
    assert _code(call(f32, 2)) == 4
    assert list(out) == [5.0] * 4
    call(buf, 1)()  # and the next call works
    assert out[0] == 10.0


@pytest.mark.gpu
def test_object_table_example():
    """examples/object_table.py: the boxes of the five planted objects come back as built -- a border point (of the thread, a stray return) lies
    within eps of a core point, so a box grows by at most eps on either side; the ground filter may take the foot of a wall --, and no tree
    is lower than its top"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("object_table", os.path.join(root, "examples", "object_table.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    rows = example.objects()
    assert len(rows) == 5 and all(r["built"] is not None for r in rows)
    for r in rows:
        assert np.allclose(r["size"][:2], r["built"][:2], atol=2.0 * example.objects_scene.EPS), r
        assert 0.5 * r["built"][2] < r["size"][2] <= r["built"][2] + 2.0 * example.objects_scene.EPS, r
    rows, tops = example.trees()
    assert len(rows) > 20
    for r in rows:
        assert r["points"] > 0 and r["height"] >= example.stand_scene.MIN_HEIGHT and r["crown_spread"] > 0.0
        assert r["height"] >= tops.heights[r["tree"]], r  # (the top is a point of its own crown)
