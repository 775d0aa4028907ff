"""The wave-folded tally of sizes and smallest members per root (tally_root, grid_index_device.hpp) at its seams, through the three calls that
end in it: pst_euclidean_clusters, pst_dbscan and pst_region_growing_from_knn.

The tally folds the lanes of a wave that share a root, for the first four distinct roots of the wave, and lets the lanes left over send their
own atomics; a lane with nothing to add carries "none".  So the cases fix the roots per wave: the points lie on the x axis at increasing x,
0.5 apart inside a group and 2 apart between groups, and the tolerance / eps is 1.  Keys are the x cell only and the sort is stable, so sorted
position equals buffer index, a wave is the indices 64 w .. 64 w + 63 and a workgroup 256 of them.  The regions get chain lists over the same
groups (ids are buffer indices there anyway).

Every test first asserts, from the restatement's labels alone, that every wave has the intended number of distinct roots -- a mis-built input
cannot pass silently -- and that part also runs without a GPU (the `oracle` parametrisation of the `api` fixture).  With the HIP library the
call's labels, sizes, masks and counts are then compared exactly against tests/cluster_ref.py, dbscan_ref.py and region_ref.py."""
import functools

import numpy as np
import pytest

import cluster_ref as CR
import dbscan_ref as DR
import region_ref as RR
from test_clusters import assert_same as assert_same_clusters, gpu_label
from test_dbscan import assert_same as assert_same_dbscan, gpu_dbscan
from test_region import PAD, Z, assert_same as assert_same_regions, gpu_from_knn

NONE = 0xFFFFFFFF
WAVE = 64
INVALID, RIM, SMOOTH = 0, 1, 2

# name: (group sizes in index order, distinct roots per wave when every group is a component)
CASES = {
    "one_group_per_wave": ([64, 64], [1, 1]),
    "four_of_16": ([16] * 8, [4, 4]),
    "fifth_root_left_over": ([13, 13, 13, 13, 12] * 2, [5, 5]),  # four leaders, then the 12 send their own
    "eight_of_8": ([8] * 16, [8, 8]),
    "singletons": ([1] * 128, [64, 64]),
    "across_a_wave": ([48, 33, 47], [2, 2]),  # the second group is 48 .. 80
    "across_a_workgroup": ([240, 33, 47], [1, 1, 1, 2, 2]),  # the second group is 240 .. 272
    "partly_filled_last_wave": ([64] + [16] * 4 + [13, 13, 13, 13, 12] + [8] * 8 + [1] * 64 + [7], [1, 4, 5, 8, 64, 1]),  # n = 327
    # an isolated point as lane 0, one between two groups, one whole wave of them, then a partly filled wave
    "isolated_points": ([1, 63, 31, 1, 32] + [1] * 64 + [20], [2, 3, 64, 1]),
}


def points_of(groups):
    """(n, 3): 0.5 apart inside a group, 2 between groups, y = z = 0.  Multiples of 0.5 below 2^10: every coordinate and distance is exact."""
    x, at = [], 0.0
    for size in groups:
        x += [at + 0.5 * j for j in range(size)]
        at = x[-1] + 2.0
    pts = np.zeros((len(x), 3))
    pts[:, 0] = x
    assert (np.diff(pts[:, 0]) > 0).all()
    return pts


def chains_of(groups):
    """(n, 1) lists: every point names its successor inside its group, the last one nobody"""
    n = sum(groups)
    knn = (np.arange(n, dtype=np.int64) + 1)[:, None]
    knn[np.cumsum(groups) - 1, 0] = PAD
    return knn


def intended_roots(groups, state=None):
    """Distinct roots per wave, from the group sizes alone.  state (per point: INVALID carries nothing and links nothing, a RIM point joins its
    successor's run when that is SMOOTH and links nothing, SMOOTH points link to a SMOOTH successor in the same group); default all SMOOTH."""
    n = sum(groups)
    state = np.full(n, SMOOTH) if state is None else state
    run = np.full(n, -1)
    at = 0
    for size in groups:
        for i in range(at, at + size):
            if state[i] == SMOOTH:
                run[i] = run[i - 1] if i > at and state[i - 1] == SMOOTH else i
        for i in range(at, at + size - 1):
            if state[i] == RIM and state[i + 1] == SMOOTH:
                run[i] = run[i + 1]
        at += size
    return [len(set(run[w:w + WAVE].tolist()) - {-1}) for w in range(0, n, WAVE)]


def roots_in_labels(labels):
    """Distinct labels per wave of an unfiltered result: a label there is a component"""
    return [len(set(labels[w:w + WAVE].tolist()) - {NONE}) for w in range(0, len(labels), WAVE)]


@functools.lru_cache(maxsize=None)
def case(name):
    groups, roots = CASES[name]
    pts = points_of(groups)
    pts.setflags(write=False)
    assert intended_roots(groups) == roots, "the table's roots per wave are those of its groups"
    return groups, roots, pts


@functools.lru_cache(maxsize=None)
def cluster_want(name, min_size):
    return CR.label(case(name)[2], 1.0, min_size=min_size, grid=False)


@pytest.mark.parametrize("name", CASES)
def test_clusters(api, name):
    groups, roots, pts = case(name)
    want = cluster_want(name, 1)
    assert roots_in_labels(want[0]) == roots and sorted(want[1].tolist()) == sorted(groups)
    if not api.is_product:
        return
    assert_same_clusters(gpu_label(api, pts, 1.0, storage="V"), want, name)
    # the groups of 12 and of 1 (and whatever else is below 13) dropped: the tally is the same, the numbering skips their roots
    filtered = cluster_want(name, 13)
    assert len(filtered[1]) == sum(size >= 13 for size in groups)
    assert_same_clusters(gpu_label(api, pts, 1.0, min_size=13, device=True), filtered, name + " filtered")


@pytest.mark.parametrize("name", CASES)
def test_dbscan(api, name):
    groups, _, pts = case(name)
    want = DR.dbscan(pts, 1.0, 2, grid=False)  # an isolated point is noise: a lane that carries "none"
    noise = np.repeat(np.array(groups) == 1, groups)
    assert roots_in_labels(want[0]) == intended_roots(groups, np.where(noise, INVALID, SMOOTH)) and np.array_equal(want[0] == NONE, noise)
    one = DR.dbscan(pts, 1.0, 1, grid=False)
    assert np.array_equal(one[0], cluster_want(name, 1)[0]) and np.array_equal(one[1], cluster_want(name, 1)[1]) and one[2].all()
    if not api.is_product:
        return
    assert_same_dbscan(gpu_dbscan(api, pts, 1.0, 2, device=True), want, name)
    assert_same_dbscan(gpu_dbscan(api, pts, 1.0, 1, storage="V"), one, name + " min_points 1")


@pytest.mark.parametrize("variant", ["smooth", "rim_in_lane_0", "invalid_wave"])
@pytest.mark.parametrize("name", CASES)
def test_regions(api, name, variant):
    groups, roots, _ = case(name)
    n = sum(groups)
    knn = chains_of(groups)
    normals = np.tile(np.array(Z), (n, 1))
    curvature = np.zeros(n)
    state = np.full(n, SMOOTH)
    if variant == "rim_in_lane_0":   # lane 0 of every wave is a rim point: it joins its successor's region, or nothing as the last of its group
        curvature[::WAVE] = 1.0
        state[::WAVE] = RIM
    elif variant == "invalid_wave":  # the second wave carries nothing at all
        normals[WAVE:2 * WAVE] = np.nan
        state[WAVE:2 * WAVE] = INVALID
    want = RR.region_growing(knn, normals, curvature, curvature_threshold=0.5)
    assert roots_in_labels(want[0]) == intended_roots(groups, state) and np.array_equal(want[2], state == SMOOTH)
    if variant == "smooth":
        assert roots_in_labels(want[0]) == roots
    if not api.is_product:
        return
    got = gpu_from_knn(api, knn, normals, curvature, curvature_threshold=0.5, device=variant == "rim_in_lane_0")
    assert_same_regions(got, want, f"{name} {variant}")
