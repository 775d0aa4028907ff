"""voxelgrid_filter at the seams of its code paths, bit for bit against the numpy restatement of tests/voxel_ref.py.

voxel.hip picks a path by the size of a voxel (48 / 49 points: lane or wave; 64 / 65 and 2048 / 2049: the three most-common forms), of a group of
64 voxels (staged through LDS up to a capacity of 1024 .. 6144 points), of the marker table (6144 markers: LDS or global) and of the key (32 / 33
bits: key type and sort); find_leaf_axis has a three-marker fast path and two fix-up loops; the run heads are found in tiles of 2048 keys, eight
per thread.  Every cloud here is built so that something sits exactly on such a seam.  Each cloud and its expectation are computed once and
shared by the oracle run, the HIP run and the stream-ordered plan; nothing is compared with a tolerance: attribute bytes, voxel count and voxel
order must be the restatement's.
"""
import numpy as np
import pytest

import voxel_ref as R
from harness import BUFFER_KINDS
from pasture_amd.algorithms import voxelgrid_filter
from pasture_amd.layout import PointLayout, attributes as A

FULL = [A.POSITION_3D, A.INTENSITY, A.RETURN_NUMBER, A.NUMBER_OF_RETURNS, A.CLASSIFICATION_FLAGS, A.SCANNER_CHANNEL, A.SCAN_DIRECTION_FLAG,
        A.EDGE_OF_FLIGHT_LINE, A.CLASSIFICATION, A.SCAN_ANGLE_RANK, A.SCAN_ANGLE, A.USER_DATA, A.POINT_SOURCE_ID, A.COLOR_RGB, A.GPS_TIME, A.NIR,
        A.POINT_ID, A.NORMAL]  # every attribute set_all_attributes knows (:478-689), packed
U8_FIRST = [A.CLASSIFICATION] + [a for a in FULL if a is not A.CLASSIFICATION]  # Position3D at byte 1: the staged fetch's aligned(1) pair load
POS_INTENSITY = [A.POSITION_3D, A.INTENSITY]
UNIT = (1.0, 1.0, 1.0)


def packed_dtype(attrs):
    names, formats, offsets, at = [], [], [], 0
    for a in attrs:
        dt = a.datatype()
        names.append(a.name())
        formats.append((dt.numpy_dtype(), (dt.num_components(),)) if dt.num_components() > 1 else dt.numpy_dtype())
        offsets.append(at)
        at += dt.size()
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": at})


class Case:
    def __init__(self, rec, leaf, attrs, populations=None):
        self.rec, self.leaf, self.attrs = rec, leaf, attrs
        self.order, self.starts, self.counts, self.markers = R.voxel_membership(rec["Position3D"], leaf)
        if populations is not None:  # the reference's own membership is the builder's
            assert np.array_equal(self.counts, populations)
        self.exp = R.numpy_voxelgrid(rec, None, leaf)
        self.rec.setflags(write=False)
        self.exp.setflags(write=False)


def stage_cap(n, n_voxels):
    """voxel_grid_reduce's LDS capacity: 1.6 x the average group of 64 voxels, within 1024 .. 6144 points, a multiple of 64."""
    groups = (n_voxels + 63) // 64
    return min(6144, max(1024, (n * 8 // 5) // groups + 63)) & ~63


def lattice_case(populations, seed, attrs=FULL, **kw):
    pos, voxel, realised = R.lattice_cloud(populations, seed, **kw)
    assert np.array_equal(realised, populations)
    rng = np.random.default_rng(seed + 1)
    rec = np.zeros(len(pos), dtype=packed_dtype(attrs))
    rec["Position3D"] = pos
    R.fill_random_attributes(rec, rng)
    R.fill_most_common_seams(rec, voxel, rng)
    return rec, voxel


# ---- the clouds ----------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4097]


def sizes_case():
    """One seam voxel per group of 64, at a different lane each time, single points around it."""
    pops = np.ones(64 * len(SIZES), dtype=np.int64)
    for g, m in enumerate(SIZES):
        pops[64 * g + (7 * g + 3) % 64] = m
    rec, voxel = lattice_case(pops, 11)
    # the most-common columns: no value holds a majority anywhere, five or more distinct values from five points on
    order, starts, counts = R.rows_of_voxels(voxel)
    rows = np.repeat(np.arange(len(counts)), counts)
    for name in R.MOST_COMMON:
        u, cnt = np.unique(rows * 131072 + rec[name][order].astype(np.int64) + 32768, return_counts=True)
        vox = u // 131072
        assert (np.maximum.reduceat(cnt, np.flatnonzero(np.r_[True, vox[1:] != vox[:-1]])) * 2 <= np.maximum(counts, 2)).all(), name
        assert (np.bincount(vox)[counts >= 5] >= 5).all(), name
    return Case(rec, UNIT, FULL, pops)


def padded_groups(groups, tail):
    """Populations of the given groups, then groups of 64 single-point voxels until the default staging capacity is 1024, then `tail` voxels."""
    pops = [m for g in groups for m in g]
    assert all(len(g) == 64 for g in groups)
    while True:
        n, nv = sum(pops) + tail, len(pops) + tail
        if (n * 8 // 5) // ((nv + 63) // 64) + 63 < 1024:
            break
        pops += [1] * 64
    pops = np.array(pops + [1] * tail, dtype=np.int64)
    assert stage_cap(int(pops.sum()), len(pops)) == 1024 and len(pops) % 64 == tail
    return pops


def group_with(base, count, odd, lane):
    g = [base] * count
    g.insert(lane, odd)
    return g


def group_case(which, tail):
    """Groups of 64 voxels whose points total cap - 1, cap, cap + 1, once as many middling voxels and once as one large voxel among single points."""
    if which == "1024":
        groups = [[1] * 64]  # (the anchor's group)
        for k, t in enumerate((1023, 1024, 1025)):
            groups.append(group_with(16, 63, t - 63 * 16, 5 * k + 1))
            groups.append(group_with(1, 63, t - 63, 9 * k + 2))
        groups.append(group_with(1, 63, 2, 33))  # 65 points, next to the groups of 64 and (tail 63) of 63: the seam of a capacity pinned to 64
        groups.append([47, 48, 49, 1000] + [1] * 60)  # over the capacity, so not staged: 47 and 48 points are a lane's loop, 49 a wave's
    elif which == "6144a":
        groups = [group_with(97, 63, t - 63 * 97, 11 * k + 4) for k, t in enumerate((6143, 6144, 6145))]
    else:
        groups = [group_with(1, 63, t - 63, 13 * k + 6) for k, t in enumerate((6143, 6144, 6145))]
    pops = padded_groups(groups, tail)
    rec, _ = lattice_case(pops, 23 + tail)
    assert len(rec) < 40_000
    return Case(rec, UNIT, FULL, pops)


def run_head_case(n):
    """Voxels that begin at chosen positions of the sorted order: around the tile seam 2048, around multiples of eight (a thread's keys), one
    voxel over two whole tiles, and heads inside the ragged last vector of a cloud whose length is no multiple of eight."""
    heads = [0, 1, 7, 8, 9, 15, 16, 17, 24, 2040, 2047, 2048, 2049, 2056, 4090, 8200, 8207, 8208, 8209, n - 12, n - 9, n - 8, n - 3, n - 1]
    assert heads[14] < 2 * 2048 and heads[15] > 4 * 2048
    pops = np.diff(np.r_[heads, n])
    rec, _ = lattice_case(pops, 31 + n % 7)
    case = Case(rec, UNIT, FULL, pops)
    assert np.array_equal(case.starts, heads)
    return case


def indexed(pos):
    """Position3D and Intensity only; the intensity is the point's index, so a misfiled point changes two voxels' averages."""
    rec = np.zeros(len(pos), dtype=packed_dtype(POS_INTENSITY))
    rec["Position3D"] = pos
    rec["Intensity"] = np.arange(len(pos)) % 65536
    return rec


def exact_marker_case():
    """Leaf 0.5 from 0: the markers 0.5, 1.0 .. 12.0 and the midpoints between them are exact.  Coordinates on every marker, on every midpoint
    (it belongs to the UPPER marker: the step back needs a strictly nearer lower one), one ulp either side of both, the minimum and the maximum."""
    markers = 0.5 * np.arange(1, 25)
    mids = markers - 0.25
    s = np.r_[0.0, 12.0, markers, mids, np.nextafter(markers, -np.inf), np.nextafter(markers[:-1], np.inf), np.nextafter(mids, -np.inf), np.nextafter(mids, np.inf)]
    pos = np.concatenate([np.stack([np.roll(s, a), np.roll(s, b), np.roll(s, c)], axis=1) for a, b, c in ((0, 37, 71), (5, 0, 101), (50, 13, 0))])
    case = Case(indexed(pos), (0.5, 0.5, 0.5), POS_INTENSITY)
    assert all(np.array_equal(m, markers) for m in case.markers)
    assert np.array_equal(R.find_leaf(mids, markers), np.arange(24)) and np.array_equal(R.find_leaf(np.nextafter(mids[1:], -np.inf), markers), np.arange(23))
    return case


def drift_case(leaf):
    """From 2^30 a leaf of about 1e-6 is 4.6 or 5.5 ulps, and every accumulated marker rounds to a whole ulp: the markers step by a different
    amount than the leaf, and find_leaf_axis's arithmetic guess runs away from the true cell -- low for one leaf, high for the other."""
    rng = np.random.default_rng(int(leaf * 1e9))
    origin = 2.0 ** 30
    pos = np.full((4000, 3), 5.0)
    pos[:, :2] = origin + rng.uniform(0.0, 2000 * leaf, size=(4000, 2))
    pos[0, :2] = origin
    case = Case(indexed(pos), (leaf, leaf, leaf), POS_INTENSITY)
    signs = set()
    for c in range(2):  # precondition: the guess, computed as the kernel does, is two or more cells off for nearly every point
        m, p = case.markers[c], pos[:, c]
        assert 1500 < len(m) < 2500
        t = (p - origin) * (1.0 / leaf)
        guess = np.where(t >= 1.0, np.minimum(t, len(m) - 1).astype(np.int64), 0)
        off = guess - np.minimum(np.searchsorted(m, p, side="left"), len(m) - 1)
        assert (np.abs(off) >= 2).mean() >= 0.9, (np.abs(off) >= 2).mean()
        signs.add(int(np.sign(off.sum())))
    case.drift = signs
    return case


def marker_total_case(total):
    """One long axis, no y markers and one z marker: `total` markers in all (the marker table moves from LDS to global memory above 6144)."""
    rng = np.random.default_rng(total)
    nx = total - 1
    x = np.r_[0.0, float(nx), 0.4, 0.5, 0.6, 1.0, 1.4, 1.5, 1.6, nx - 1.6, nx - 1.5, nx - 1.0, nx - 0.6, nx - 0.5, nx - 0.4, rng.uniform(0, nx, 3000)]
    pos = np.stack([x, np.full(len(x), 3.0), np.where(np.arange(len(x)) % 2 == 0, 0.0, 0.9)], axis=1)
    case = Case(indexed(pos), UNIT, POS_INTENSITY)
    assert [len(m) for m in case.markers] == [nx, 0, 1] and sum(len(m) for m in case.markers) == total
    return case


def bits_for(count):
    """voxel_grid_build: bits of an axis field holding the indices 0 .. count - 1 (one bit at least)."""
    b = 1
    while b < 21 and (1 << b) < count:
        b += 1
    return b


def key_bits_case(counts, end_bit, n_random):
    """Exactly counts[c] markers on axis c; all eight corners are occupied, so the highest index of every field appears next to 0 and to the
    highest index of its neighbours."""
    rng = np.random.default_rng(sum(counts))
    top = np.array(counts, dtype=np.float64)
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64) * top
    pos = np.concatenate([corners, corners * 0.999 + 0.0001, rng.uniform(0, 1, (n_random, 3)) * top])
    case = Case(indexed(pos), UNIT, POS_INTENSITY)
    assert [len(m) for m in case.markers] == list(counts) and sum(bits_for(c) for c in counts) == end_bit
    return case


GPS_SCENARIOS = 7
NAN_PAYLOADS = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)


def values_case():
    """Special values in voxels of 3, 60 and 300 points, once in a group small enough to be staged and once in a group that a fourth voxel of 700
    points pushes over the capacity (3: a lane's loop; 60 and 300: a wave's).  Every point but the anchor has z = -0.0."""
    groups = [[1] * 64]
    for s in range(GPS_SCENARIOS):
        groups.append([3, 60, 300] + [1] * 61)
        groups.append([3, 60, 300, 700] + [1] * 60)
    pops = padded_groups(groups, 0)
    rec, voxel = lattice_case(pops, 41, dims=(8, 1), flat_z=-0.0)
    order, starts, counts = R.rows_of_voxels(voxel)
    rng = np.random.default_rng(42)
    for s in range(GPS_SCENARIOS):
        for g in (1 + 2 * s, 2 + 2 * s):
            for v in range(64 * g, 64 * g + 3):
                m = int(counts[v])
                pts = order[starts[v]:starts[v] + m]  # ascending index = the order the reference visits them in
                gps = rng.uniform(1.0, 100.0, m)
                if s == 0:
                    gps = -gps                                           # all negative -> 0.0
                elif s in (1, 2, 3):
                    gps[(0, m // 2, m - 1)[s - 1]] = NAN_PAYLOADS[(s + v) % 4]  # NaN first / in the middle / last: never wins
                elif s == 4:
                    gps[m // 3], gps[m - 1] = np.inf, NAN_PAYLOADS[1]    # -> +inf
                elif s == 5:
                    gps[:] = -np.inf                                     # -> 0.0
                else:
                    gps[:] = -0.0                                        # -> +0.0
                rec["GpsTime"][pts] = gps
                pid = rng.integers(0, 2 ** 52, m, dtype=np.uint64)
                if s % 3 == 0:
                    pid[m // 2] = 2 ** 53 + 1                            # `as f64` rounds to 2^53
                elif s % 3 == 1:
                    pid[m - 1] = 2 ** 64 - 1                             # `as f64` is 2^64; `as u64` saturates
                else:
                    pid[0], pid[1] = 2 ** 63, 2 ** 63 + 1                # both 2^63 as f64
                rec["PointID"][pts] = pid
                if s % 2 == 0:
                    rec["Intensity"][pts] = 65535
                    rec["ColorRGB"][pts] = 65535
                nrm = rng.normal(size=(m, 3)).astype(np.float32)
                if s % 3 == 0:
                    nrm[:] = np.float32(3e38) * np.array([1, -1, 1], dtype=np.float32)  # the f64 sum of 300 of them is finite; so is the average as f32
                elif s % 3 == 1:
                    nrm[m // 2, 0] = np.nan
                else:
                    nrm[:] = -0.0
                rec["Normal"][pts] = nrm
    case = Case(rec, UNIT, FULL, pops)
    cap = stage_cap(len(rec), len(pops))
    for s in range(GPS_SCENARIOS):
        assert counts[64 * (1 + 2 * s):64 * (2 + 2 * s)].sum() <= cap < counts[64 * (2 + 2 * s):64 * (3 + 2 * s)].sum()
    # what the values must come to, stated once by hand
    e = case.exp
    v0 = 64 * 1
    assert e["GpsTime"][v0:v0 + 3].view(np.uint64).tolist() == [0, 0, 0] and np.isinf(e["GpsTime"][64 * 9:64 * 9 + 3]).all()
    assert e["GpsTime"][64 * 13:64 * 13 + 3].view(np.uint64).tolist() == [0, 0, 0] and not np.isnan(e["GpsTime"]).any()
    assert e["PointID"][v0:v0 + 3].tolist() == [2 ** 53] * 3 and e["PointID"][64 * 3:64 * 3 + 3].tolist() == [2 ** 64 - 1] * 3
    assert e["PointID"][64 * 5:64 * 5 + 3].tolist() == [2 ** 63] * 3
    assert (e["Intensity"][v0:v0 + 3] == 65535).all() and (e["ColorRGB"][v0:v0 + 3] == 65535).all()
    assert np.array_equal(e["Normal"][v0:v0 + 3], np.tile(np.float32(3e38) * np.array([1, -1, 1], dtype=np.float32), (3, 1)))
    assert np.isnan(e["Normal"][64 * 3:64 * 3 + 3, 0]).all() and (e["Normal"][64 * 5:64 * 5 + 3].view(np.uint32) == 0).all()
    assert (e["Position3D"][1:, 2].view(np.uint64) == 0).all()  # the centroid of -0.0 coordinates is +0.0
    return case


BUILDERS = {
    "sizes": sizes_case,
    "g1024-0": lambda: group_case("1024", 0), "g1024-1": lambda: group_case("1024", 1), "g1024-63": lambda: group_case("1024", 63),
    "g6144a-1": lambda: group_case("6144a", 1), "g6144b-63": lambda: group_case("6144b", 63),
    "heads-0": lambda: run_head_case(5 * 2048), "heads-1": lambda: run_head_case(5 * 2048 + 1), "heads-2047": lambda: run_head_case(5 * 2048 + 2047),
    "exact": exact_marker_case, "drift-1.3": lambda: drift_case(1.3e-6), "drift-1.1": lambda: drift_case(1.1e-6),
    "markers-6143": lambda: marker_total_case(6143), "markers-6144": lambda: marker_total_case(6144), "markers-6145": lambda: marker_total_case(6145),
    "bits-32": lambda: key_bits_case((2048, 2048, 1024), 32, 3000), "bits-33": lambda: key_bits_case((2048, 2048, 1025), 33, 3000),
    "bits-16": lambda: key_bits_case((16, 16, 16), 12, 600), "bits-17x": lambda: key_bits_case((17, 16, 16), 13, 600),
    "bits-17y": lambda: key_bits_case((16, 17, 16), 13, 600), "bits-17z": lambda: key_bits_case((16, 16, 17), 13, 600),
    "values": values_case,
}
_CASES = {}


def case_of(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def assert_same_cloud(filtered, exp, attrs):
    assert filtered.len() == len(exp)
    for a in attrs:
        got, want = raw(filtered.view_attribute(a)), raw(exp[a.name()])
        if not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).any(axis=1))
            raise AssertionError(f"{a.name()}: {len(bad)} of {len(exp)} voxels differ, the first is voxel {bad[0]}: "
                                 f"{filtered.view_attribute(a)[bad[0]]!r} for {exp[a.name()][bad[0]]!r}")


def run(api, name, kinds, attrs=None):
    case = case_of(name)
    attrs = attrs or case.attrs
    layout = PointLayout.from_attributes_packed(attrs, 1, api=api)
    rec = case.rec
    if attrs is not case.attrs:  # the same points in another record layout
        rec = np.zeros(len(case.rec), dtype=packed_dtype(attrs))
        for n in rec.dtype.names:
            rec[n] = case.rec[n]
    assert layout.numpy_record_dtype() == rec.dtype
    src = BUFFER_KINDS[kinds[0]].from_numpy(rec, layout)
    filtered = BUFFER_KINDS[kinds[1]].new_from_layout(layout)
    voxelgrid_filter(src, *case.leaf, filtered)
    assert_same_cloud(filtered, case.exp, attrs)


# ---- the restatement's own primitives against plain loops ----------------------------------------------------------------------------------
def test_restatement_primitives_are_the_plain_loops():
    rng = np.random.default_rng(5)
    counts = np.array([1, 7, 64, 300, 2, 1, 1000])
    starts = np.r_[0, np.cumsum(counts)[:-1]]
    vals = np.stack([rng.uniform(-1e6, 1e6, counts.sum()) * 10.0 ** rng.integers(-8, 8, counts.sum()), rng.integers(0, 65536, counts.sum()).astype(np.float64)], axis=1)
    got = R.sequential_sums(vals, starts, counts)
    pairwise_differs = False
    for v, (s, m) in enumerate(zip(starts, counts)):
        for c in range(2):
            acc = 0.0
            for x in vals[s:s + m, c]:
                acc = acc + float(x)
            assert got[v, c] == acc
            pairwise_differs = pairwise_differs or np.sum(vals[s:s + m, c]) != acc
    assert pairwise_differs  # (the data can tell the two apart)
    pool = vals[:, 0].copy()
    pool[starts[1]:starts[1] + 7] = [-3.0, np.nan, -0.0, -np.inf, -1.0, np.nan, -2.0]
    pool[starts[2]] = np.nan
    pool[starts[4]:starts[4] + 2] = [np.nan, np.nan]
    pool[starts[5]] = -0.0
    got = R.max_pool(pool, starts)
    for v, (s, m) in enumerate(zip(starts, counts)):
        cur = 0.0
        for x in pool[s:s + m]:
            if x > cur:
                cur = float(x)
        assert got[v] == cur and np.signbit(got[v]) == np.signbit(cur)
    # find_leaf :21-52 as the loop it is
    markers = R.axis_markers(0.0, 5.0, 0.5)
    p = np.r_[markers, markers - 0.25, np.nextafter(markers - 0.25, -np.inf), np.nextafter(markers, np.inf)[:-1], 0.0, 5.0, np.nan, rng.uniform(0, 5, 50)]
    want = []
    for x in p:
        i = 0
        while markers[i] < x:
            i += 1
        if i > 0 and x - markers[i - 1] < markers[i] - x:
            i -= 1
        want.append(i)
    assert np.array_equal(R.find_leaf(p, markers), want)
    # most common: highest count, then the smallest value -- signed values by their numeric order
    vals = np.array([5, 5, 3, 3, 9, -128, 127, 127, -128, 0, 65535, 1, 1, 2])
    assert R.most_common(vals, np.array([0] * 5 + [1] * 4 + [2, 3] + [4] * 3)).tolist() == [3, -128, 0, 65535, 1]
    with pytest.raises(AssertionError):
        R.most_common(vals, np.array([0] * 5 + [1] * 4 + [2, 3] + [4] * 3), forbid_ties=True)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("m", [2, 3, 5, 6, 7, 48, 64, 65, 129, 2049])
def test_mode_seam_column_is_what_it_says(m, mode):
    col = R.mode_seam_column(m, -128, 127, mode, (-128, 127), np.random.default_rng(m))
    vals, cnt = np.unique(col, return_counts=True)
    by = dict(zip(vals.tolist(), cnt.tolist()))
    assert len(col) == m and max(cnt) * 2 <= max(m, 2) and len(vals) >= min(m, 5)
    if mode == 0 or m < 6:
        assert by[-128] == by[127] == max(cnt)
    else:
        assert by[127] == by[-128] + 1 == max(cnt) and sorted(cnt)[-2] == by[-128] and col[m - 1 if mode == 1 or m <= 64 else 64] == 127


# ---- the product and the oracle against it --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", ["HH", "VV", "HV", "VH"])
def test_voxel_size_seams(api, kinds):
    run(api, "sizes", kinds)


def test_voxel_size_seams_with_position_at_an_odd_offset(api):
    run(api, "sizes", "VV", U8_FIRST)


@pytest.mark.parametrize("kinds", ["HH", "VV"])
@pytest.mark.parametrize("name", ["g1024-0", "g1024-1", "g1024-63", "g6144a-1", "g6144b-63"])
def test_group_seams(api, name, kinds):
    run(api, name, kinds)


@pytest.mark.parametrize("kinds", ["HH", "VV"])
@pytest.mark.parametrize("name", ["heads-0", "heads-1", "heads-2047"])
def test_run_head_seams(api, name, kinds):
    run(api, name, kinds)


@pytest.mark.parametrize("kinds", ["HH", "VV"])
def test_coordinates_on_markers_and_midpoints(api, kinds):
    run(api, "exact", kinds)


@pytest.mark.parametrize("name", ["drift-1.3", "drift-1.1"])
def test_markers_that_drift_from_the_arithmetic_guess(api, name):
    run(api, name, "HH")
    assert case_of("drift-1.3").drift | case_of("drift-1.1").drift == {-1, 1}  # one leaf's guess is low, the other's high: both fix-up loops


@pytest.mark.parametrize("name", ["markers-6143", "markers-6144", "markers-6145"])
def test_marker_table_seam(api, name):
    run(api, name, "VV")


@pytest.mark.parametrize("name", ["bits-32", "bits-33", "bits-16", "bits-17x", "bits-17y", "bits-17z"])
def test_key_width_seams(api, name):
    run(api, name, "HH")


@pytest.mark.parametrize("kinds", ["HH", "VV"])
def test_special_values(api, kinds):
    run(api, "values", kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", ["HH", "VV"])
@pytest.mark.parametrize("name", ["sizes", "g1024-0", "g1024-63", "g6144a-1", "g6144b-63"])
def test_plan_at_the_seams(hip, name, kinds):
    """The stream-ordered form (fixed big-voxel grid, device-side count, the plan's own staging capacity) against the restatement itself."""
    import torch
    from pasture_amd.algorithms import VoxelGridPlan
    case = case_of(name)
    layout = PointLayout.from_attributes_packed(case.attrs, 1, api=hip)
    size = layout.size_of_point_entry()
    src = BUFFER_KINDS[kinds[0]].from_numpy(case.rec, layout)
    plan = VoxelGridPlan(src, *case.leaf)
    first, total = 3, 3 + plan.max_voxels
    out = BUFFER_KINDS[kinds[1]].new_from_layout(layout)
    out.resize(total)
    out.set_point_range(range(0, total), np.full((total, size), 0xAB, dtype=np.uint8))
    cs = torch.zeros(2, dtype=torch.int64, device="cuda")
    plan.filter_async(src, out, first, cs.data_ptr())
    torch.cuda.synchronize()
    count, status = (int(x) for x in cs.tolist())
    assert status == 0 and count == len(case.exp) <= plan.max_voxels
    got = out.get_point_range(range(0, total))
    want = raw(case.exp)
    assert want.shape == (count, size)
    for a in layout.attributes():
        o, sz = a.offset(), a.size()
        assert np.array_equal(got[first:first + count, o:o + sz], want[:, o:o + sz]), a.name()
    assert (got[:first] == 0xAB).all() and (got[first + count:] == 0xAB).all()
    plan.destroy()
