"""Numpy restatement of minimum-distance (Poisson-disk) subsampling (include/pasture_amd.h, "Minimum-distance subsampling").

    conflict      finite i, j:  (dx*dx + dy*dy) + dz*dz <= r2,  r2 = radius * radius, every operation a separately rounded f64 operation
    priority key  shuffled: splitmix64(seed ^ i); index order: i
    kept set      the sequential greedy pass in ascending key order: keep a finite point iff no kept point conflicts with it

greedy_mask walks the points in key order and looks for kept points in a dict of cells; greedy_mask_brute tests every kept point; the
synchronous simulation (synchronous_states) decides, round by round, every point all of whose smaller-key conflicts were decided the round
before -- its final states are the greedy ones and its number of rounds bounds the device's launches.  No scipy."""
import numpy as np

SHUFFLED, INDEX_ORDER = 0, 1
_ORDERS = {"shuffled": SHUFFLED, "index": INDEX_ORDER, SHUFFLED: SHUFFLED, INDEX_ORDER: INDEX_ORDER}


def splitmix64(x):
    """The finaliser of the header, on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def priorities(order, seed, n, first=0):
    """uint64 (n,): the keys of buffer indices first .. first + n - 1 (the index wraps at 2^64)."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64) + np.uint64(first & 0xFFFFFFFFFFFFFFFF)
    if _ORDERS[order] == INDEX_ORDER:
        return i
    return splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ i)


def conflicts(P, i, js, r2):
    """bool per j in js: does point j conflict with point i -- the header's expression and association on float64 arrays"""
    dx, dy, dz = P[js, 0] - P[i, 0], P[js, 1] - P[i, 1], P[js, 2] - P[i, 2]
    return (dx * dx + dy * dy) + dz * dz <= r2


def _prepare(P, radius):
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(-1, 3))
    finite = np.isfinite(P).all(axis=1)
    return P, finite, np.float64(radius) * np.float64(radius)


def _cells(P, finite, radius, limit=None):
    """int64 (n, 3): cell numbers >= 1 on a grid whose edge is a thousandth above the radius (doubled until no axis has more than `limit`
    cells): conflicting points are at most one cell apart on every axis, with a margin far above any rounding of the quotient"""
    cells = np.zeros((len(P), 3), dtype=np.int64)
    if not finite.any():
        return cells
    lo = P[finite].min(axis=0)
    extent = P[finite].max(axis=0) - lo
    edge = radius * 1.001
    while limit is not None and (extent / edge).max() >= limit:
        edge *= 2.0
    cells[finite] = np.floor((P[finite] - lo) / edge).astype(np.int64) + 1
    return cells


def greedy_mask(P, radius, keys):
    """uint8 (n,): the kept set.  Candidates come from a dict cell -> kept points of that cell (kept points are more than a radius apart, so
    every list is short)."""
    P, finite, r2 = _prepare(P, radius)
    keys = np.asarray(keys, dtype=np.uint64)
    mask = np.zeros(len(P), dtype=np.uint8)
    cells = _cells(P, finite, radius)
    kept_in = {}
    stencil = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    for i in np.argsort(keys, kind="stable"):
        if not finite[i]:
            continue
        cx, cy, cz = (int(v) for v in cells[i])
        cand = []
        for a, b, c in stencil:
            got = kept_in.get((cx + a, cy + b, cz + c))
            if got:
                cand.extend(got)
        if cand and conflicts(P, i, np.array(cand, dtype=np.int64), r2).any():
            continue
        mask[i] = 1
        kept_in.setdefault((cx, cy, cz), []).append(int(i))
    return mask


def greedy_mask_brute(P, radius, keys):
    """The same pass with every kept point a candidate: no grid at all."""
    P, finite, r2 = _prepare(P, radius)
    mask = np.zeros(len(P), dtype=np.uint8)
    kept = []
    for i in np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable"):
        if finite[i] and not (kept and conflicts(P, i, np.array(kept, dtype=np.int64), r2).any()):
            mask[i] = 1
            kept.append(int(i))
    return mask


def conflict_pairs(P, radius):
    """int64 (m, 2): every ordered pair (a, b), a != b, of finite points that conflict.  The points are sorted by a packed cell key with x
    lowest; each of the nine (y, z) rows of a point's stencil is one key range, found with searchsorted."""
    P, finite, r2 = _prepare(P, radius)
    idx = np.flatnonzero(finite)
    if len(idx) < 2:
        return np.zeros((0, 2), dtype=np.int64)
    cells = _cells(P, finite, radius, limit=1 << 19)[idx]
    K = int(cells.max()) + 2  # cell numbers 1 .. K - 2: a neighbour's number never leaves 0 .. K - 1, and K^3 < 2^60
    key = (cells[:, 2] * K + cells[:, 1]) * K + cells[:, 0]
    by_key = np.argsort(key, kind="stable")
    skey, sidx = key[by_key], idx[by_key]
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            row = skey + (dz * K + dy) * K
            lo, hi = np.searchsorted(skey, row - 1, "left"), np.searchsorted(skey, row + 1, "right")
            count = hi - lo
            total = int(count.sum())
            if total == 0:
                continue
            a = np.repeat(np.arange(len(skey)), count)
            b = np.arange(total) - np.repeat(np.cumsum(count) - count, count) + np.repeat(lo, count)
            a, b = sidx[a], sidx[b]
            keep = a != b
            a, b = a[keep], b[keep]
            dx, dyy, dzz = P[b, 0] - P[a, 0], P[b, 1] - P[a, 1], P[b, 2] - P[a, 2]
            hit = (dx * dx + dyy * dyy) + dzz * dzz <= r2
            out.append(np.stack([a[hit], b[hit]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def synchronous_states(P, radius, keys):
    """(uint8 (n,) final states: 0 not finite, 1 kept, 2 rejected; rounds; undecided points after every round).  One round: every undecided
    point looks at the states its smaller-key conflicts had BEFORE the round -- rejected if one is kept, kept if none is undecided."""
    P, finite, _ = _prepare(P, radius)
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(P)
    pr = conflict_pairs(P, radius)
    a, b = pr[:, 0], pr[:, 1]
    earlier = keys[b] < keys[a]
    a, b = a[earlier], b[earlier]  # b is a conflict of a with a smaller key
    state = np.zeros(n, dtype=np.uint8)
    undecided = finite.copy()
    rounds, history = 0, []
    while undecided.any():
        rounds += 1
        sees_kept = np.bincount(a, weights=(state[b] == 1), minlength=n) > 0
        sees_undecided = np.bincount(a, weights=undecided[b], minlength=n) > 0
        state[undecided & sees_kept] = 2
        state[undecided & ~sees_kept & ~sees_undecided] = 1
        undecided = finite & (state == 0)
        history.append(int(undecided.sum()))
    return state, rounds, history


def synchronous_rounds(P, radius, keys):
    """The number of rounds of the synchronous simulation: an upper bound on the launches of any schedule that reads states at least as
    fresh (0 for a cloud without a finite point)."""
    return synchronous_states(P, radius, keys)[1]
