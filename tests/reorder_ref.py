"""The numpy restatement of the gather by index and of the device sort orders (include/pasture_amd.h, "Gather by index and sort orders"):
the key functions exactly as defined there, np.argsort(key, kind="stable"), the Morton key with np.floor and the same clamps, splitmix64,
and the gather as fancy indexing on record bytes."""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------------- attribute keys

def attribute_keys(values, descending=False):
    """The unsigned sort keys of a 1-d array of one numeric dtype, as wide as the dtype."""
    v = np.ascontiguousarray(values)
    width = v.dtype.itemsize
    U = np.dtype(f"<u{width}")
    ones = U.type(np.iinfo(U).max)
    sign = U.type(1 << (8 * width - 1))
    nan = np.zeros(v.shape, dtype=bool)
    if v.dtype.kind == "u":
        key = v.astype(U)
    elif v.dtype.kind == "i":
        key = v.view(U) ^ sign
    elif v.dtype.kind == "f":
        bits = v.view(U).copy()
        bits[bits == sign] = 0  # -0.0 is +0.0
        key = np.where((bits & sign) != 0, ~bits, bits | sign)
        nan = np.isnan(v)
        key[nan] = ones
    else:
        raise TypeError(v.dtype)
    if descending:
        key = np.where(nan, key, ~key)
    return key.astype(U)


def argsort_attribute(values, descending=False):
    return np.argsort(attribute_keys(values, descending), kind="stable").astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------- Morton keys

NONFINITE_KEY = np.uint64(1 << 63)


def morton_bits(dims, bits):
    return bits if bits else (31 if dims == 2 else 21)


def morton_keys(points, dims=3, bits=0):
    """uint64 key of every point of an (n, 3) float64 array"""
    P = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    bits = morton_bits(dims, bits)
    lim = float(2 ** bits)
    finite = np.isfinite(P).all(axis=1)
    keys = np.zeros(len(P), dtype=np.uint64)
    if finite.any():
        mn, mx = P[finite].min(axis=0), P[finite].max(axis=0)
        with np.errstate(all="ignore"):
            inv = lim / (mx - mn)
        inv = np.where((mx != mn) & np.isfinite(inv), inv, 0.0)
        with np.errstate(all="ignore"):
            t = (P - mn) * inv  # two separately rounded operations
            c = np.where(t >= lim, lim - 1.0, np.where(t >= 0.0, np.floor(t), 0.0))  # (a NaN t fails both comparisons: 0)
        c = np.where(finite[:, None], c, 0.0).astype(np.uint64)
        for a in range(dims):
            for i in range(bits):
                keys |= ((c[:, a] >> np.uint64(i)) & np.uint64(1)) << np.uint64(dims * i + a)
    keys[~finite] = NONFINITE_KEY
    return keys


def morton_order(points, dims=3, bits=0):
    return np.argsort(morton_keys(points, dims, bits), kind="stable").astype(np.uint32)


# -------------------------------------------------------------------------------------------------------------------------------- shuffle

def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def shuffle_keys(n, seed):
    return splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ np.arange(n, dtype=np.uint64))


def shuffle_order(n, seed):
    return np.argsort(shuffle_keys(n, seed), kind="stable").astype(np.uint32)


def invert(order, n=None):
    order = np.asarray(order, dtype=np.int64)
    inverse = np.zeros(len(order) if n is None else n, dtype=np.uint32)
    inverse[order] = np.arange(len(order), dtype=np.uint32)
    return inverse


# --------------------------------------------------------------------------------------------------------------------------------- gather

def attribute_byte_mask(layout):
    """bool per byte of a record: the byte belongs to an attribute (not padding)"""
    mask = np.zeros(layout.size_of_point_entry(), dtype=bool)
    for a in layout.attributes():
        mask[a.offset():a.offset() + a.size()] = True
    return mask


def gather(src_records, indices, dst_records, dst_first=0, byte_mask=None, skip_out_of_range=False):
    """dst[dst_first + j] = src[indices[j]] on (n, size) uint8 record arrays; byte_mask: only these bytes of a record are written (the
    pairings that leave record padding alone).  skip_out_of_range: the stream-ordered form; returns (records, skipped)."""
    src = np.asarray(src_records, dtype=np.uint8)
    out = np.array(dst_records, dtype=np.uint8, copy=True)
    idx = np.asarray(indices).astype(np.uint64)
    ok = idx < np.uint64(len(src))
    assert skip_out_of_range or ok.all()
    j = np.flatnonzero(ok)
    picked = src[idx[j].astype(np.int64)]
    if byte_mask is None:
        out[dst_first + j] = picked
    else:
        rows = out[dst_first + j]
        rows[:, byte_mask] = picked[:, byte_mask]
        out[dst_first + j] = rows
    return (out, int((~ok).sum())) if skip_out_of_range else out
