"""The progressive morphological ground filter restated in numpy (the definition of include/pasture_amd.h, "Ground classification").

Everything is a minimum, a maximum or one f64 addition, which numpy evaluates with the same roundings as the device: the mask, the count and the
three rasters are compared with np.array_equal, no tolerance anywhere.

erode / dilate are written twice: `*_brute` is the definition (every cell looks at its whole clipped square), `erode` / `dilate` slide along the
two axes in turn.  The CPU tests hold them against each other; the large cases use the second."""
import numpy as np

MAX_WINDOWS = 32
MAX_CELLS = 1 << 28


def schedule(cell_size=1.0, max_window_size=33.0, slope=1.0, initial_distance=0.15, max_distance=2.5, exponential=True, base=2):
    """(half-widths, thresholds): h_k = base^k or (k + 1) base, w_k = 2 h_k + 1, th_0 = initial_distance,
    th_k = min(max_distance, slope * (w_k - w_(k-1)) * cell_size + initial_distance); ends after the first w_k * cell_size >= max_window_size."""
    hs, ths = [], []
    w_before = None
    k = 0
    while True:
        if k == MAX_WINDOWS:
            raise ValueError("more than 32 windows")
        h = base ** k if exponential else (k + 1) * base
        w = 2 * h + 1
        th = np.float64(initial_distance)
        if k > 0:
            th = min(np.float64(max_distance), np.float64(slope) * np.float64(w - w_before) * np.float64(cell_size) + np.float64(initial_distance))
        hs.append(h)
        ths.append(float(th))
        if np.float64(w) * np.float64(cell_size) >= max_window_size:
            break
        w_before = w
        k += 1
    return np.array(hs, dtype=np.uint32), np.array(ths, dtype=np.float64)


def cells_of(pts, cell_size):
    """(finite, row, col, rows, cols, (x0, y0)): row and col for the finite points only, in their order; zeros without a finite point"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    finite = np.isfinite(pts).all(axis=1)
    if not finite.any():
        return finite, np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0, 0, (0.0, 0.0)
    x, y = pts[finite, 0], pts[finite, 1]
    x0, y0 = x.min(), y.min()
    col = ((x - x0) / np.float64(cell_size)).astype(np.uint32)
    row = ((y - y0) / np.float64(cell_size)).astype(np.uint32)
    return finite, row, col, int(row.max()) + 1, int(col.max()) + 1, (float(x0), float(y0))


def min_raster(pts, cell_size):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    finite, row, col, rows, cols, _ = cells_of(pts, cell_size)
    z0 = np.full(rows * cols, np.inf)
    np.minimum.at(z0, row.astype(np.int64) * cols + col, pts[finite, 2])
    return z0.reshape(rows, cols)


def erode_brute(a, h):
    rows, cols = a.shape
    out = np.empty_like(a)
    for r in range(rows):
        for c in range(cols):
            out[r, c] = a[max(r - h, 0):r + h + 1, max(c - h, 0):c + h + 1].min()
    return out


def dilate_brute(a, h):
    rows, cols = a.shape
    out = np.empty_like(a)
    for r in range(rows):
        for c in range(cols):
            w = a[max(r - h, 0):r + h + 1, max(c - h, 0):c + h + 1]
            w = w[w < np.inf]
            out[r, c] = w.max() if w.size else np.inf
    return out


def _slide(a, h, fold):
    out = a.copy()
    for axis in (0, 1):
        src = out.copy()
        for d in range(1, min(h, a.shape[axis] - 1) + 1):
            lo = [slice(None)] * 2
            hi = [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, -d), slice(d, None)
            lo, hi = tuple(lo), tuple(hi)
            out[hi] = fold(out[hi], src[lo])
            out[lo] = fold(out[lo], src[hi])
    return out


def erode(a, h):
    return _slide(np.asarray(a, dtype=np.float64), int(h), np.minimum)


def dilate(a, h):
    a = np.asarray(a, dtype=np.float64)
    out = _slide(np.where(a < np.inf, a, -np.inf), int(h), np.maximum)
    return np.where(out == -np.inf, np.inf, out)


def ground(pts, hs, ths, cell_size):
    """(mask uint8, count, {min_z, opened, limit}) for the windows (hs, ths); without a finite point the rasters are empty"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    finite, row, col, rows, cols, _ = cells_of(pts, cell_size)
    mask = np.zeros(len(pts), dtype=np.uint8)
    if not finite.any():
        empty = np.zeros((0, 0))
        return mask, 0, {"min_z": empty, "opened": empty, "limit": empty}
    z0 = min_raster(pts, cell_size)
    z, limit = z0, np.full_like(z0, np.inf)
    for h, th in zip(hs, ths):
        z = dilate(erode(z, h), h)
        limit = np.minimum(limit, z + np.float64(th))
    mask[finite] = pts[finite, 2] <= limit[row, col]
    return mask, int(mask.sum()), {"min_z": z0, "opened": z, "limit": limit}


def scene(n=60000, seed=5):
    """The recorded scene: rolling terrain over 64 x 64 with a roof and a pole.  Returns (points, is_roof, is_pole)."""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * 64.0
    noise = rng.normal(0.0, 0.02, n)
    lift = rng.uniform(1.0, 6.0, n)
    x, y = xy[:, 0], xy[:, 1]
    z = 0.05 * x + 1.5 * np.sin(x / 9.0) * np.cos(y / 11.0) + noise
    roof = (x > 20) & (x < 27) & (y > 30) & (y < 36)
    pole = (x - 45.0) ** 2 + (y - 12.0) ** 2 < 0.4 ** 2
    z = np.where(roof, z + 4.0, z)
    z = np.where(pole, z + lift, z)
    return np.column_stack([x, y, z]), roof, pole
