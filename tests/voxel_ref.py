"""voxelgrid_filter (pasture-algorithms/src/voxel_grid.rs:21-689) restated with numpy, and a builder of clouds whose voxels have chosen sizes
(test helper, numpy only).

The restatement, per target attribute:
  * cells: create_markers_for_axis (:55-83) accumulates `curr += leaf` from the cloud's minimum; find_leaf (:21-52) takes the first marker that is
    not below the coordinate, then steps back when the marker before it is STRICTLY nearer.  A NaN coordinate stays in cell 0.
  * voxels come out in (x, y, z) cell order; the points of a voxel are visited in ascending index.
  * averages (:332-440): `sum += v as f64` one point after the other from 0.0, then `sum / n as f64`, then Rust `as` into the attribute's type.
  * max-pool (:169-219): `cur = 0.0; if x > cur { cur = x }` -- NaN never wins, all-negative input and -0.0 give +0.0 -- then Rust `as`.
  * most common (:222-329): the value with the highest count.  The reference breaks ties by HashMap iteration order (random per process); this
    project's contract is "highest count, then smallest value", for signed types the numerically smallest.  The two bool attributes count the
    raw u8 values and store `value != 0`.
"""
import math

import numpy as np

from rust_as_ref import rust_as_array

AVERAGE_VEC = ("Position3D", "ColorRGB", "Normal")
AVERAGE_NUM = ("Intensity", "NIR")
MAX_POOL = ("ClassificationFlags", "GpsTime", "PointID")
MOST_COMMON_BOOL = ("ScanDirectionFlag", "EdgeOfFlightLine")
MOST_COMMON = ("ReturnNumber", "NumberOfReturns", "ScannerChannel", "ScanDirectionFlag", "EdgeOfFlightLine", "Classification", "ScanAngleRank",
               "ScanAngle", "UserData", "PointSourceID")


def axis_markers(mn, mx, leaf):
    """create_markers_for_axis: accumulated sums, not mn + k * leaf."""
    markers = []
    cur = float(mn)
    while cur < mx:
        cur += float(leaf)
        markers.append(cur)
    return np.array(markers, dtype=np.float64)


def find_leaf(p, markers):
    """find_leaf for one axis and many coordinates."""
    p = np.asarray(p, dtype=np.float64)
    if len(markers) == 0:
        return np.zeros(p.shape, dtype=np.int64)
    i = np.searchsorted(markers, p, side="left")  # first marker with !(marker < p); searchsorted files NaN behind everything
    i = np.where(np.isnan(p), 0, np.minimum(i, len(markers) - 1)).astype(np.int64)
    prev = markers[np.maximum(i - 1, 0)]
    with np.errstate(invalid="ignore"):
        back = (i > 0) & (p - prev < markers[i] - p)
    return i - back


def voxel_membership(pos, leaf):
    """-> (order, starts, counts, markers): `order` lists the point indices voxel after voxel, voxels in (x, y, z) cell order and ascending
    index inside a voxel; voxel v owns order[starts[v] : starts[v] + counts[v]]; markers = the three marker arrays."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    idx = np.zeros((n, 3), dtype=np.int64)
    markers = []
    for c in range(3):
        col = pos[:, c]
        ok = ~np.isnan(col)  # calculate_bounds compares strictly: NaN is never a bound
        markers.append(axis_markers(col[ok].min(), col[ok].max(), leaf[c]))
        idx[:, c] = find_leaf(col, markers[c])
    order = np.lexsort((np.arange(n), idx[:, 2], idx[:, 1], idx[:, 0]))
    keys = idx[order]
    starts = np.flatnonzero(np.r_[True, (np.diff(keys, axis=0) != 0).any(axis=1)])
    counts = np.diff(np.r_[starts, n])
    return order, starts, counts, markers


def sequential_sums(values, starts, counts):
    """values: (n, k) f64, voxel after voxel.  -> (voxels, k): per voxel and column `acc = 0.0; for x in rows: acc += x`, the rows in order.
    Step j adds row j of every voxel that has one -- an elementwise f64 addition, so each voxel's chain is the plain loop's (np.sum and
    np.add.reduceat add pairwise and round differently)."""
    values = np.asarray(values, dtype=np.float64)
    by_size = np.argsort(-counts, kind="stable")
    s, c = starts[by_size], counts[by_size]
    acc = np.zeros((len(starts), values.shape[1]), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(int(c[0]) if len(c) else 0):
            k = int(np.searchsorted(-c, -j, side="left"))  # the voxels with more than j points are a prefix
            acc[:k] += values[s[:k] + j]
    out = np.empty_like(acc)
    out[by_size] = acc
    return out


def max_pool(values, starts):
    """`cur = 0.0; if x > cur { cur = x }` per voxel.  fmax skips NaN; whatever is not above 0.0 (negatives, -0.0, NaN only) leaves +0.0."""
    m = np.fmax.reduceat(np.asarray(values, dtype=np.float64), starts)
    with np.errstate(invalid="ignore"):
        return np.where(m > 0.0, m, 0.0)


def most_common(values, voxel_of_row, forbid_ties=False):
    """values: integers in [-32768, 65535], voxel after voxel; voxel_of_row ascending.  -> per voxel the value with the highest count, the
    smallest such value on a tie."""
    key = voxel_of_row.astype(np.int64) * 131072 + (np.asarray(values).astype(np.int64) + 32768)
    u, cnt = np.unique(key, return_counts=True)
    vox, val = u // 131072, u % 131072 - 32768
    order = np.lexsort((val, -cnt, vox))
    head = np.r_[True, vox[order][1:] != vox[order][:-1]]
    if forbid_ties:
        second = np.flatnonzero(~head)
        second = second[head[second - 1]]  # the runner-up of every voxel that has one
        assert not (cnt[order][second] == cnt[order][second - 1]).any(), "test data must not contain most-common ties"
    return val[order][head]


def _rust_as(avg, dtype):
    """Rust `as` of f64 results, element by element through rust_as_ref (each distinct bit pattern once)."""
    flat = np.ascontiguousarray(avg, dtype=np.float64).reshape(-1)
    bits, inverse = np.unique(flat.view(np.uint64), return_inverse=True)
    return rust_as_array(bits.view(np.float64), dtype)[inverse.reshape(-1)].reshape(np.shape(avg))


def numpy_voxelgrid(rec, layout, leaf, forbid_ties=False):
    """The filtered cloud as a record array of rec's dtype, one record per occupied voxel.  `layout` names the attributes to reduce (None: all
    of rec's).  forbid_ties: assert that no voxel has two most-common candidates (data meant to be valid for the reference's HashMap too)."""
    names = [a.name() for a in layout.attributes()] if layout is not None else list(rec.dtype.names)
    order, starts, counts, _ = voxel_membership(rec["Position3D"], leaf)
    voxel_of_row = np.repeat(np.arange(len(starts)), counts)
    out = np.zeros(len(starts), dtype=rec.dtype)
    n_pts = counts.astype(np.float64)
    sums = [n for n in names if n in AVERAGE_VEC or n in AVERAGE_NUM]
    if sums:
        cols = np.concatenate([rec[n][order].astype(np.float64).reshape(len(rec), -1) for n in sums], axis=1)
        with np.errstate(over="ignore", invalid="ignore"):
            avg = sequential_sums(cols, starts, counts) / n_pts[:, None]
        at = 0
        for n in sums:
            width = 3 if n in AVERAGE_VEC else 1
            a = avg[:, at:at + width] if width == 3 else avg[:, at]
            out[n] = a if n == "Position3D" else _rust_as(a, rec.dtype[n].base)
            at += width
    for n in names:
        if n in MAX_POOL:
            out[n] = _rust_as(max_pool(rec[n][order].astype(np.float64), starts), rec.dtype[n])
        elif n in MOST_COMMON:
            best = most_common(rec[n][order], voxel_of_row, forbid_ties)
            out[n] = (best != 0) if n in MOST_COMMON_BOOL else best.astype(rec.dtype[n])
        elif n not in sums:
            raise AssertionError(f"no reduction rule for {n}")
    return out


# ---- clouds with chosen voxel populations --------------------------------------------------------------------------------------------------
def lattice_cloud(populations, seed, dims=(8, 8), flat_z=None):
    """Voxel v gets populations[v] points and sits in cell v of an x-major lattice of dims = (ny, nz) cells per x slab.  The leaf is 1.0 and one
    anchor point lies at the origin, so the markers are the integers 1.0, 2.0 .. exactly and cell i of an axis is centred on i + 1; every other
    point lies within +-0.25 of its markers.  The anchor falls into cell (0, 0, 0) and counts as one of voxel 0's points.  flat_z: every point
    but the anchor has this z (nz = 1, no z markers).  The input order is a seeded permutation, so a voxel's points are scattered and the sorted
    index list is a true gather.
    -> (pos (n, 3), voxel_of_point (n,), realised): realised[v] = points placed in voxel v."""
    populations = np.asarray(populations, dtype=np.int64)
    assert len(populations) and (populations >= 1).all()
    ny, nz = (dims[0], 1) if flat_z is not None else dims
    rng = np.random.default_rng(seed)
    v = np.repeat(np.arange(len(populations)), populations)[1:]  # (voxel 0 gives one of its points to the anchor)
    cell = np.stack([v // (ny * nz), (v // nz) % ny, v % nz], axis=1).astype(np.float64)
    pos = cell + 1.0 + rng.uniform(-0.25, 0.25, size=cell.shape)
    if flat_z is not None:
        pos[:, 2] = flat_z
    pos = np.concatenate([np.zeros((1, 3)), pos])
    voxel = np.concatenate([[0], v])
    perm = rng.permutation(len(pos))
    pos, voxel = pos[perm], voxel[perm]
    return pos, voxel, np.bincount(voxel, minlength=len(populations))


def rows_of_voxels(voxel):
    """-> (order, starts, counts) of a voxel_of_point array: order[starts[v] + r] is the point at sorted position r of voxel v."""
    order = np.argsort(voxel, kind="stable")
    counts = np.bincount(voxel)
    return order, np.r_[0, np.cumsum(counts)[:-1]], counts


def fill_random_attributes(rec, rng):
    """Full-range random values for whatever averaged / max-pooled attributes rec has."""
    n = len(rec)
    names = rec.dtype.names
    for name in ("Intensity", "NIR"):
        if name in names:
            rec[name] = rng.integers(0, 65536, n)
    if "ColorRGB" in names:
        rec["ColorRGB"] = rng.integers(0, 65536, (n, 3))
    if "GpsTime" in names:
        rec["GpsTime"] = rng.uniform(-5, 100, n)
    if "ClassificationFlags" in names:
        rec["ClassificationFlags"] = rng.integers(0, 256, n)
    if "PointID" in names:
        rec["PointID"] = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    if "Normal" in names:
        rec["Normal"] = rng.normal(size=(n, 3)).astype(np.float32)


TIE_PAIRS = {"ScanAngleRank": [(-1, 0), (-128, 127)], "ScanAngle": [(-32768, 32767)], "PointSourceID": [(0, 65535)],
             "ScanDirectionFlag": [(0, 1)], "EdgeOfFlightLine": [(0, 1)]}


def mode_seam_column(m, lo, hi, mode, domain, rng):
    """The m values of one voxel at its sorted positions 0 .. m - 1, with no majority and at least five distinct values from m = 5 on.
    mode 0: lo and hi tie for the highest count (lo must win).  mode 1 / 2: hi leads lo by ONE, and one of its occurrences sits at position
    m - 1 (the last, partial chunk of 64) / at position 64 (the first of the second chunk; m - 1 when the voxel is shorter).  Voxels too small for
    a lead next to three other values (m < 6) get the tie."""
    near = 1 if mode != 0 and m >= 6 else 0
    if m < 5:
        c, rest = (1, m - 2) if m >= 2 else (0, 1)
    else:
        c = min(m // 3, (m - 3 - near) // 2)
        rest = m - 2 * c - near
    per = max(1, c - 1)  # a filler stays below the pair (or ties with everything when the pair itself has one occurrence each)
    f = 0 if rest == 0 else max(min(3, rest), math.ceil(rest / per))
    fillers = np.zeros(0, dtype=np.int64)
    while len(fillers) < f:
        cand = rng.integers(domain[0], domain[1] + 1, size=f + 8)
        fillers = np.unique(np.r_[fillers, cand[(cand != lo) & (cand != hi)]])
    fillers = rng.permutation(fillers)[:f]
    col = np.r_[np.full(c, lo), np.full(c + near, hi) if m >= 2 else [], np.repeat(fillers, [rest // f + (i < rest % f) for i in range(f)])].astype(np.int64)
    assert len(col) == m
    col = rng.permutation(col)
    if near:
        want = m - 1 if mode == 1 or m <= 64 else 64
        have = int(np.flatnonzero(col == hi)[0])
        col[have], col[want] = col[want], col[have]
    return col


def fill_most_common_seams(rec, voxel, rng):
    """Every most-common attribute rec has, voxel by voxel (mode_seam_column); the mode cycles with voxel and attribute, so every voxel size meets
    every mode in some attribute.  Pairs: TIE_PAIRS, else 0 / 255 and a random pair by turns."""
    order, starts, counts = rows_of_voxels(voxel)
    for ai, name in enumerate(n for n in MOST_COMMON if n in rec.dtype.names):
        info = np.iinfo(rec.dtype[name])
        col = rng.integers(info.min, info.max + 1, len(rec)).astype(np.int64)  # (voxels of one point)
        for v in np.flatnonzero(counts >= 2):
            pairs = TIE_PAIRS.get(name)
            if pairs:
                lo, hi = pairs[v % len(pairs)]
            elif v % 2:
                lo, hi = int(info.min), int(info.max)
            else:
                lo, hi = sorted(int(x) for x in rng.choice(info.max - info.min + 1, 2, replace=False) + info.min)
            m = int(counts[v])
            col[order[starts[v]:starts[v] + m]] = mode_seam_column(m, lo, hi, (v + ai) % 3, (int(info.min), int(info.max)), rng)
        rec[name] = col
