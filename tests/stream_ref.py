"""The fused Vec3f64 stream of pasture_amd/csrc/stream.hip and stream_tile.hpp, restated in numpy (test helper, numpy only).

mode bits as in kernels.hpp: 1 = affine, 2 = write the target, 4 = bounds.  The stream sees a range of n points as 3 n doubles; the kernels move
16-byte vectors, so a range that starts 8 bytes off a 16-byte boundary (vec_first = 1) has one ragged double in front, and
n_vec = (3 n - vec_first) // 2 vectors in its body with 0 or 1 ragged double behind.

The three launch shapes, as (vectors per tile, vectors per row = threads per block):"""
import numpy as np

from minmax_ref import F64_MAX, bounds_ref

SHAPE_WRITE = (768, 256)          # modes 2, 3: stream_shape() in stream.hip, 3 loads x 256 threads, one tile per block
SHAPE_WRITE_BOUNDS = (1536, 512)  # modes 6, 7: stream_shape(), 3 loads x 512 threads, one tile per block
SHAPE_READ = (1536, 256)          # modes 4, 5: kStreamLoads (6) x kBlock (256) on a persistent grid of 4 blocks per CU
FOLD_TWO_LEVEL_ABOVE = 4096       # launch_finalize: more records than this fold through kFoldBlocks (128) first-level records
FOLD_BLOCKS = 128


def shape_of(mode):
    if mode & 2:
        return SHAPE_WRITE_BOUNDS if mode & 4 else SHAPE_WRITE
    return SHAPE_READ


def rows_of(shape):
    return shape[0] // shape[1]


def n_vec_of(n_points, vec_first):
    """16-byte vectors in the body of a range of n_points whose first double is vec_first doubles off a 16-byte boundary"""
    return (3 * n_points - vec_first) // 2 if n_points else 0


def seeds():
    return np.full(3, F64_MAX), np.full(3, -F64_MAX)


def stream_ref(doubles_bits, n_points, scale, offset, mode):
    """doubles_bits: the 3 n source doubles as uint64.  -> (target bits as uint64, or None for a mode that does not write; (min, max) of the
    values the mode folds, the seeds for no points or all-NaN components, or None for a mode without bounds).
    The affine is p * scale, then + offset: two roundings, what -ffp-contract=off and the fp contract(off) pragmas give."""
    src = np.ascontiguousarray(doubles_bits, dtype=np.uint64)
    assert src.shape == (3 * n_points,)
    values = src.view(np.float64).reshape(n_points, 3)
    if mode & 1:
        with np.errstate(all="ignore"):
            moved = values * np.asarray(scale, dtype=np.float64)
            moved = moved + np.asarray(offset, dtype=np.float64)
    else:
        moved = values
    target = np.ascontiguousarray(moved).reshape(-1).view(np.uint64).copy() if mode & 2 else None
    bounds = None
    if mode & 4:
        bounds = bounds_ref(moved) if n_points else seeds()
    return target, bounds


def _counts_with(n_vec, vec_first):
    """every n whose range at this phase has exactly n_vec vectors (3 n - vec_first is 2 n_vec or 2 n_vec + 1)"""
    return [n for n in range((2 * n_vec) // 3, (2 * n_vec + 2) // 3 + 2) if n_vec_of(n, vec_first) == n_vec]


def seam_targets(tile_vec, blk):
    t = tile_vec
    return sorted({0, 1, 63, 64, 65, blk - 1, blk, blk + 1, t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 3 * t, 8 * t - 1, 8 * t, 8 * t + 1, 16 * t + 1})


def seam_counts(tile_vec, blk):
    """{vec_first: [(n_points, n_vec), ...]}: for every vector count of seam_targets() the point counts n that give exactly that many vectors at
    that phase; where none does (3 n cannot be 2 n_vec + vec_first or one more), the nearest reachable vector count on each side."""
    out = {}
    for vec_first in (0, 1):
        found = {}
        for target in seam_targets(tile_vec, blk):
            hits = _counts_with(target, vec_first)
            if hits:
                found.update({n: target for n in hits})
                continue
            for step in (-1, 1):
                v = target + step
                while v >= 0 and not _counts_with(v, vec_first):
                    v += step
                if v >= 0:
                    found.update({n: v for n in _counts_with(v, vec_first)})
        out[vec_first] = sorted(found.items())
    return out


def lane_doubles(shape, vec_first, tile, lane):
    """[(index of the double in the range, row j, half h)] of the doubles thread `lane` of the block that owns `tile` loads, in load order"""
    tile_vec, blk = shape
    return [(vec_first + 2 * (tile * tile_vec + lane + j * blk) + h, j, h) for j in range(rows_of(shape)) for h in (0, 1)]
