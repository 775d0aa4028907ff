"""Host reference of the compaction (pasture_amd/csrc/filter.hip) for tests/test_filter_seams.py, numpy only: the per-tile counts of a byte
mask, their exclusive sum, the compacted records -- and deterministic builders of masks with a stated number of matches in every tile.
The contract: mask[i] != 0 keeps point i, whatever the byte's value."""
import numpy as np

TILE = 2048
HOSTILE = (1, 2, 0x7F, 0x80, 0x81, 0xFE, 0xFF)  # the byte values a popcount-of-high-bits trick can get wrong: carries, the high bit alone, all bits
POSITIONS = ("random", "first", "last", "first_and_last", "run")


def tile_counts(mask, tile=TILE):
    """number of non-zero bytes of every tile (the last one ragged), uint32"""
    m = np.asarray(mask).view(np.uint8).reshape(-1)
    n = m.size
    full = n // tile
    counts = np.count_nonzero(m[:full * tile].reshape(full, tile), axis=1).astype(np.uint32)
    if n > full * tile:
        counts = np.append(counts, np.uint32(np.count_nonzero(m[full * tile:])))
    return counts.astype(np.uint32)


def tile_offsets(counts):
    """exclusive sum in uint64 with the total appended: len(counts) + 1 values"""
    out = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=out[1:])
    return out


def compact(rec, mask):
    return rec[np.asarray(mask).view(np.uint8).reshape(-1) != 0]


def compact_limited(rec, mask, limit):
    return compact(rec, mask)[:limit]


def _tile_on(kind, counts, tile, rng):
    """bool [len(counts), tile]: row t has counts[t] True entries, placed by `kind`; vectorised for every kind but "random" """
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 1)
    if (counts < 0).any() or (counts > tile).any():
        raise ValueError(f"a tile of {tile} bytes holds 0..{tile} matches")
    j = np.arange(tile, dtype=np.int64)[None, :]
    if kind == "first":
        return j < counts
    if kind == "last":
        return j >= tile - counts
    if kind == "first_and_last":
        head = (counts + 1) // 2
        return (j < head) | (j >= tile - (counts - head))
    if kind == "run":
        start = rng.integers(0, tile - counts + 1)
        return (j >= start) & (j < start + counts)
    if kind == "random":
        on = np.zeros((len(counts), tile), dtype=bool)
        for t, c in enumerate(counts[:, 0]):
            on[t, rng.permutation(tile)[:c]] = True
        return on
    raise ValueError(kind)


def mask_with_counts(counts, tail=0, rng=None, values=(1,), positions="random", tail_count=0, tile=TILE):
    """A uint8 mask of len(counts) full tiles and a ragged tail of `tail` bytes; tile t holds exactly counts[t] non-zero bytes and the tail
    `tail_count` (at random places).  positions: one of POSITIONS for every tile, or one entry per tile.  The non-zero bytes take their values
    from `values`, drawn with `rng` (a numpy Generator; default: seeded from the arguments).  Thousands of tiles: every kind but "random" is
    built without a loop over the tiles."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if rng is None:
        rng = np.random.default_rng([len(counts), tail, int(counts.sum())])
    values = np.asarray(values, dtype=np.uint8)
    if values.size == 0 or (values == 0).any():
        raise ValueError("values must be non-zero")
    if tail_count > tail:
        raise ValueError(f"{tail_count} matches do not fit a tail of {tail} bytes")
    if isinstance(positions, str):
        on = _tile_on(positions, counts, tile, rng)
    else:
        if len(positions) != len(counts):
            raise ValueError("one position kind per tile")
        on = np.concatenate([_tile_on(k, counts[t:t + 1], tile, rng) for t, k in enumerate(positions)]) if len(counts) else np.zeros((0, tile), bool)
    on = on.reshape(-1)
    if tail:
        t_on = np.zeros(tail, dtype=bool)
        t_on[rng.permutation(tail)[:tail_count]] = True
        on = np.concatenate([on, t_on])
    mask = values[rng.integers(0, len(values), on.size, dtype=np.uint8)] if len(values) > 1 else np.full(on.size, values[0], dtype=np.uint8)
    mask[~on] = 0
    return mask
