"""The sorts and scans of pasture_amd/csrc/radix_sort.hip, called directly (tests/cpp/sort_hooks.cpp forwards to the pstk:: functions of
device_sort.hpp) and compared bit for bit with numpy: the stable LSD sort of (u32 | u64 key, u32 value) pairs, the exclusive sum of u32 into u64
and the in-place suffix minimum.  Every comparison is exact.

Reference of a sort: order = np.argsort(keys & mask, kind="stable") with mask = 2**end_bit - 1; the sorted keys are keys[order] -- the FULL
key: bits at and above end_bit take no part in the order and come through unchanged -- the values vals[order], or `order` itself when the sort
numbers the pairs (iota).

Every array the library may write and the scratch block sit between guards of a sentinel value which must be intact afterwards; the scratch is
filled with 0xA5 bytes before a call (the products reuse theirs uncleared).  Shapes are the smallest that reach a path: the u32 tile is 8192
pairs, the u64 tile 4096; one pass up to 9 bits, three up to 27, four up to 32, ceil(end_bit / 9) beyond; radix_scan_rows_kernel walks more
than 512 tiles in a second round, scan_sums_kernel more than 512 blocks of 4096 elements."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import sort_hooks
from sort_hooks import HIP_ERROR_INVALID_VALUE, HIP_SUCCESS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {32: 8192, 64: 4096}
KEY = {32: np.uint32, 64: np.uint64}
GUARD = 64                       # elements before and behind every device array
SCRATCH_GUARD = 256              # bytes before and behind the scratch (keeps its 256-byte alignment)
SENTINEL = {4: 0xC0DEC0DE, 8: 0xC0DEC0DEC0DEC0DE}  # the guards
UNWRITTEN = {4: 0x0BADF00D, 8: 0x0BADF00D0BADF00D}  # what an output holds before the call
NOT_READ = 0xDEADBEEF            # vals_in of a sort that numbers the pairs itself


@pytest.fixture(scope="module")
def hooks():
    return sort_hooks.load()  # (raises "run build()" when the library is missing: never a skip)


def split_bits(end_bit):
    """the first pass's share of a 32-bit-key sort: end_bit split evenly (the larger shares first) over 1, 3 or 4 passes"""
    passes = 1 if end_bit <= 9 else 3 if end_bit <= 27 else 4
    return -(-end_bit // passes)


# ---- CPU: the host side of the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 8191, 8192, 8193, 9 * 8192])
def test_first_pass_fields(hooks, n):
    tmp = 0x7000_0000_1000  # (never dereferenced: host code)
    for end_bit in range(0, 33):
        counts, tiles, bits, tile_size = hooks.radix_sort_first_pass(tmp, n, end_bit)
        assert (counts, tiles, bits, tile_size) == (tmp, -(-n // 8192), split_bits(end_bit), 8192), end_bit


SIZE_QUERY_N = [0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 9 * 8192 + 1, 513 * 8192 + 5, 10 ** 8, 0xFFFFFFEF]


@pytest.mark.parametrize("width", [32, 64])
def test_sort_size_query(hooks, width):
    sort = hooks.radix_sort_pairs_u32 if width == 32 else hooks.radix_sort_pairs_u64
    for end_bit in (0, 1, 9, 10, 27, 28, 32) + ((33, 64) if width == 64 else ()):
        last = 0
        for n in SIZE_QUERY_N:
            need = ctypes.c_size_t(12345)
            assert sort(0, need, 0, 0, 0, 0, n, end_bit) == HIP_SUCCESS  # (null arrays: a query that touched them would crash)
            tiles = -(-n // TILE[width])
            assert need.value >= 512 * max(tiles, 1) * 4 + 2 * 512 * 4, (n, end_bit)
            assert need.value >= last, (n, end_bit)
            last = need.value


def test_scan_size_query(hooks):
    for scan in (lambda need, n: hooks.exclusive_sum_u32_u64(0, need, 0, 0, n), lambda need, n: hooks.suffix_min_u32(0, need, 0, n)):
        last = 0
        for n in SIZE_QUERY_N:
            need = ctypes.c_size_t(12345)
            assert scan(need, n) == HIP_SUCCESS
            assert need.value != 12345 and need.value >= last, n
            last = need.value


def test_unsupported_sizes_are_refused(hooks):
    assert hooks.radix_sort_pairs_supported(100, 32) and hooks.radix_sort_pairs_supported(0xFFFFFFEF, 0)
    assert not hooks.radix_sort_pairs_supported(100, 33)
    assert not hooks.radix_sort_pairs_supported(0xFFFFFFF0, 32)
    for sort, n, end_bit in ((hooks.sort_pairs_u32, 100, 33), (hooks.sort_pairs_u32, 0xFFFFFFF0, 32), (hooks.sort_pairs_u64, 100, 65),
                             (hooks.sort_pairs_u64, 0xFFFFFFF0, 64)):
        need = ctypes.c_size_t(12345)
        assert sort(0, need, 0, 0, 0, 0, n, end_bit) == HIP_ERROR_INVALID_VALUE  # (a size query: nothing can have been launched)
        assert need.value == 12345


# ---- GPU: device arrays between guards ----------------------------------------------------------------------------------------------------------
class Dev:
    """[GUARD + off sentinels | payload | GUARD sentinels] in one torch allocation; `off` elements shift the payload off its 16-byte alignment"""

    def __init__(self, payload, off=0):
        import torch
        payload = np.ascontiguousarray(payload)
        self.dtype, self.n, self.start = payload.dtype, payload.size, GUARD + off
        self.host = np.full(self.start + self.n + GUARD, SENTINEL[self.dtype.itemsize], dtype=self.dtype)
        self.host[self.start:self.start + self.n] = payload
        self.t = torch.from_numpy(self.host.view(np.uint8)).cuda()
        self.ptr = self.t.data_ptr() + self.start * self.dtype.itemsize
        assert self.t.data_ptr() % 256 == 0

    def fetch(self):
        """the payload now; the guards must be what was uploaded"""
        whole = self.t.cpu().numpy().view(self.dtype)
        end = self.start + self.n
        assert np.array_equal(whole[:self.start], self.host[:self.start]), "written before the array"
        assert np.array_equal(whole[end:], self.host[end:]), "written behind the array"
        return whole[self.start:end]

    def untouched(self):
        return np.array_equal(self.fetch(), self.host[self.start:self.start + self.n])


class Scratch:
    def __init__(self, nbytes):
        import torch
        self.nbytes = nbytes
        self.host = np.full(SCRATCH_GUARD + nbytes + SCRATCH_GUARD, 0x5C, dtype=np.uint8)
        self.host[SCRATCH_GUARD:SCRATCH_GUARD + nbytes] = 0xA5
        self.t = torch.from_numpy(self.host).cuda()
        self.ptr = self.t.data_ptr() + SCRATCH_GUARD
        assert self.ptr % 256 == 0

    def write_head(self, words):
        import torch
        raw = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8))
        assert raw.numel() <= self.nbytes
        self.t[SCRATCH_GUARD:SCRATCH_GUARD + raw.numel()].copy_(raw)

    def fetch(self):
        whole = self.t.cpu().numpy()
        end = SCRATCH_GUARD + self.nbytes
        assert np.array_equal(whole[:SCRATCH_GUARD], self.host[:SCRATCH_GUARD]), "written before the scratch"
        assert np.array_equal(whole[end:], self.host[end:]), "written behind the scratch"
        return whole[SCRATCH_GUARD:end]

    def untouched(self):
        return bool((self.fetch() == 0xA5).all())


def _sync(stream):
    import torch
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()  # (that stream only)


def _side_stream():
    import torch
    return torch.cuda.Stream()


def _after_uploads(stream):
    import torch
    stream.wait_stream(torch.cuda.current_stream())


def rand_bits(rng, n, bits, dtype):
    if bits == 0:
        return np.zeros(n, dtype=dtype)
    return rng.integers(0, (1 << bits) - 1, n, dtype=np.uint64, endpoint=True).astype(dtype)


def expected_sort(keys, vals, end_bit):
    mask = keys.dtype.type((1 << end_bit) - 1)
    order = np.argsort(keys & mask, kind="stable")
    return keys[order], (order.astype(np.uint32) if vals is None else vals[order])


def sort_call(hooks, keys):
    return hooks.radix_sort_pairs_u32 if keys.dtype == np.uint32 else hooks.radix_sort_pairs_u64


def query_sort_bytes(hooks, keys, n, end_bit):
    need = ctypes.c_size_t(0)
    assert sort_call(hooks, keys)(0, need, 0, 0, 0, 0, n, end_bit) == HIP_SUCCESS
    return need.value


def first_pass_histogram(hooks, scratch, keys, end_bit):
    """what a caller's key kernel leaves in the scratch: counts[digit * tiles + tile] over the lowest `bits` bits, one np.bincount per tile"""
    n = keys.size
    counts, tiles, bits, tile_size = hooks.radix_sort_first_pass(scratch.ptr, n, end_bit)
    # (only ever the true histogram in the layout the sort expects: anything else makes its scatter write out of range)
    assert (counts, tiles, bits, tile_size) == (scratch.ptr, -(-n // 8192), split_bits(end_bit), 8192)
    low = keys & np.uint32((1 << bits) - 1)
    hist = np.zeros((1 << bits, tiles), dtype=np.uint32)
    for t in range(tiles):
        hist[:, t] = np.bincount(low[t * tile_size:(t + 1) * tile_size], minlength=1 << bits)
    assert int(hist.sum()) == n
    return hist.ravel()


def run_sort(hooks, keys, vals, end_bit, *, hist=False, off=0, stream=None, scratch=None, short_by=0, n_arg=None):
    """vals None: the sort numbers the pairs (iota) and vals_in holds NOT_READ.  Returns the call's status, the output payloads and the arrays."""
    n = keys.size if n_arg is None else n_arg
    iota = vals is None
    width = keys.dtype.itemsize
    need = query_sort_bytes(hooks, keys, n, end_bit)
    if scratch is None:
        scratch = Scratch(need)
    assert scratch.nbytes >= need
    ka, kb = Dev(keys, off), Dev(np.full(keys.size, UNWRITTEN[width], dtype=keys.dtype), off)
    va = Dev(np.full(keys.size, NOT_READ, dtype=np.uint32) if iota else vals, off)
    vb = Dev(np.full(keys.size, UNWRITTEN[4], dtype=np.uint32), off)
    if off:
        assert ka.ptr % 16 == width and kb.ptr % 16 == width and va.ptr % 16 == 4 and vb.ptr % 16 == 4
    if hist:
        scratch.write_head(first_pass_histogram(hooks, scratch, keys, end_bit))
    if stream is not None:
        _after_uploads(stream)
    handle = 0 if stream is None else stream.cuda_stream
    bytes_ = ctypes.c_size_t(scratch.nbytes - short_by if short_by else scratch.nbytes)
    if keys.dtype == np.uint32:
        rc = hooks.radix_sort_pairs_u32(scratch.ptr, bytes_, ka.ptr, kb.ptr, va.ptr, vb.ptr, n, end_bit, handle, iota, hist)
    else:
        assert not iota and not hist
        rc = hooks.radix_sort_pairs_u64(scratch.ptr, bytes_, ka.ptr, kb.ptr, va.ptr, vb.ptr, n, end_bit, handle)
    _sync(stream)
    return types.SimpleNamespace(rc=rc, keys=kb.fetch(), vals=vb.fetch(), ka=ka, kb=kb, va=va, vb=vb, scratch=scratch)


def check_sort(hooks, keys, vals, end_bit, **kw):
    r = run_sort(hooks, keys, vals, end_bit, **kw)
    assert r.rc == HIP_SUCCESS
    exp_keys, exp_vals = expected_sort(keys, vals, end_bit)
    assert np.array_equal(r.keys, exp_keys), "sorted keys"
    assert np.array_equal(r.vals, exp_vals), "sorted values (stable order)"
    r.scratch.fetch()  # (guards)
    if end_bit <= 9:   # one pass: the first pair of buffers is only read -- and vals_in of an iota sort not even that
        assert r.ka.untouched() and r.va.untouched()
    else:              # (scratch of the later passes: contents free, guards not)
        r.ka.fetch(), r.va.fetch()
    return r


def rand_vals(rng, n):
    return rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint64, endpoint=True).astype(np.uint32)


# ---- sizes x widths --------------------------------------------------------------------------------------------------------------------------
U32_SIZES = [0, 1, 2, 63, 64, 65, 8191, 8192, 8193, 7 * 8192 + 3, 8 * 8192, 9 * 8192 + 1, 17 * 8192 + 100]
U32_WIDTHS = [0, 1, 8, 9, 10, 18, 26, 27, 28, 31, 32]
U64_SIZES = [0, 1, 63, 4095, 4096, 4097, 9 * 4096 + 1, 17 * 4096 + 100]
U64_WIDTHS = [1, 9, 10, 27, 28, 32, 33, 36, 37, 45, 46, 54, 55, 63, 64]
# every width at 1 tile, 9 tiles + 1 and 17 tiles + 100 (the pass-count seams and the copy-back of an even number of passes); the other sizes
# (tile edges, the grid's rounding to a multiple of 8 and its early return) at one width per pass count and the seams' upper sides
U32_CASES = [(n, e) for n in U32_SIZES for e in (U32_WIDTHS if n in (8192, 9 * 8192 + 1, 17 * 8192 + 100) else (0, 1, 9, 10, 27, 28, 32))]
U64_CASES = [(n, e) for n in U64_SIZES for e in (U64_WIDTHS if n in (4096, 9 * 4096 + 1, 17 * 4096 + 100) else (1, 10, 28, 33, 46, 64))]


@pytest.mark.gpu
@pytest.mark.parametrize("iota", [False, True])
@pytest.mark.parametrize("n,end_bit", U32_CASES)
def test_sort_u32(hooks, n, end_bit, iota):
    """Keys are random in all 32 bits: below end_bit they decide the order (for a small end_bit with many equal keys, whose input order must
    survive), at and above it they must be ignored and preserved.  end_bit 0 is the regression case of a defect this test found: the sort
    took bit 0 for its one pass, so random keys came out grouped by their lowest bit instead of in input order."""
    rng = np.random.default_rng([32, n, end_bit, int(iota)])
    keys = rand_bits(rng, n, 32, np.uint32)
    check_sort(hooks, keys, None if iota else rand_vals(rng, n), end_bit)


@pytest.mark.gpu
@pytest.mark.parametrize("n,end_bit", U64_CASES)
def test_sort_u64(hooks, n, end_bit):
    rng = np.random.default_rng([64, n, end_bit])
    keys = rand_bits(rng, n, 64, np.uint64)
    if n % 2:  # (half of the cases: keys below 2^end_bit, as the products make them)
        keys &= np.uint64((1 << end_bit) - 1)
    check_sort(hooks, keys, rand_vals(rng, n), end_bit)


@pytest.mark.gpu
@pytest.mark.parametrize("width,end_bit", [(32, 27), (64, 39)])
def test_sort_of_more_than_512_tiles(hooks, width, end_bit):
    """513 tiles + 5 pairs: radix_scan_rows_kernel scans a digit's row in rounds of 512 tiles and carries the sum into the second round"""
    n = 513 * TILE[width] + 5
    rng = np.random.default_rng([width, n])
    keys = rand_bits(rng, n, end_bit, KEY[width])
    check_sort(hooks, keys, None if width == 32 else rand_vals(rng, n), end_bit)


# ---- key patterns ----------------------------------------------------------------------------------------------------------------------------
def make_keys(pattern, n, end_bit, dtype, rng):
    width = np.dtype(dtype).itemsize * 8
    mask = (1 << end_bit) - 1
    if pattern == "uniform":
        return rand_bits(rng, n, end_bit, dtype)
    if pattern == "few":  # at most 32 distinct values
        return rand_bits(rng, 32, end_bit, dtype)[rng.integers(0, 32, n)]
    if pattern == "equal":
        return np.full(n, rand_bits(rng, 1, end_bit, dtype)[0], dtype=dtype)
    if pattern == "equal_mask":
        return np.full(n, mask, dtype=dtype)
    if pattern == "all_bits_set":  # the value a partial last tile is padded with, among other keys (end_bit = the key's width)
        assert end_bit == width
        keys = rand_bits(rng, n, end_bit, dtype)
        keys[rng.random(n) < 0.5] = mask
        keys[-1] = mask
        return keys
    if pattern == "top_bit":  # two values that differ in bit end_bit - 1 only
        low = rand_bits(rng, 1, end_bit - 1, dtype)[0]
        return low | (rng.integers(0, 2, n).astype(dtype) << dtype(end_bit - 1))
    if pattern in ("ascending", "descending"):
        i = np.arange(n, dtype=np.uint64)
        keys = (i * np.uint64(mask // n) if mask >= n else i * np.uint64(mask) // np.uint64(n - 1)).astype(dtype)  # strictly / weakly ascending
        return keys if pattern == "ascending" else keys[::-1].copy()
    if pattern == "high_bits":  # few distinct low parts under random bits at and above end_bit: ignored, preserved, equal low parts in input order
        assert end_bit < width
        return make_keys("few", n, end_bit, dtype, rng) | (rand_bits(rng, n, width - end_bit, dtype) << dtype(end_bit))
    raise ValueError(pattern)


def pattern_cases(width):
    tile, full, below = TILE[width], ((9, 27, 32) if width == 32 else (9, 39, 64)), ((9, 27, 31) if width == 32 else (9, 39, 63))
    cases = []
    for n in (tile + 1, 9 * tile + 1):
        cases += [(p, n, e) for p in ("uniform", "few", "equal", "equal_mask", "top_bit", "ascending", "descending") for e in full]
        cases += [("all_bits_set", n, width)] + [("high_bits", n, e) for e in below]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n,end_bit", pattern_cases(32))
def test_sort_u32_key_patterns(hooks, pattern, n, end_bit):
    rng = np.random.default_rng([32, n, end_bit, len(pattern)])
    keys = make_keys(pattern, n, end_bit, np.uint32, rng)
    check_sort(hooks, keys, rand_vals(rng, n), end_bit)
    check_sort(hooks, keys, None, end_bit)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n,end_bit", pattern_cases(64))
def test_sort_u64_key_patterns(hooks, pattern, n, end_bit):
    rng = np.random.default_rng([64, n, end_bit, len(pattern)])
    keys = make_keys(pattern, n, end_bit, np.uint64, rng)
    check_sort(hooks, keys, rand_vals(rng, n), end_bit)


# ---- arrays off the 16-byte boundary, streams, scratch -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("iota", [False, True])
@pytest.mark.parametrize("end_bit", [9, 27, 32])
@pytest.mark.parametrize("tiles,extra", [(1, 0), (8, 0), (9, 1)])
def test_sort_u32_unaligned_arrays(hooks, tiles, extra, end_bit, iota):
    """all four arrays start 4 bytes behind a 16-byte boundary: full tiles then take the element loop of the histogram kernel"""
    n = tiles * 8192 + extra
    rng = np.random.default_rng([32, n, end_bit, 4])
    check_sort(hooks, rand_bits(rng, n, 32, np.uint32), None if iota else rand_vals(rng, n), end_bit, off=1)


@pytest.mark.gpu
@pytest.mark.parametrize("end_bit", [9, 39, 64])
@pytest.mark.parametrize("tiles,extra", [(1, 0), (8, 0), (9, 1)])
def test_sort_u64_unaligned_arrays(hooks, tiles, extra, end_bit):
    n = tiles * 4096 + extra
    rng = np.random.default_rng([64, n, end_bit, 8])
    check_sort(hooks, rand_bits(rng, n, 64, np.uint64), rand_vals(rng, n), end_bit, off=1)


@pytest.mark.gpu
def test_sort_and_scans_on_a_side_stream(hooks):
    """issued on a torch side stream, synchronised on that stream only"""
    rng = np.random.default_rng(77)
    n = 9 * 8192 + 1
    check_sort(hooks, rand_bits(rng, n, 32, np.uint32), None, 27, stream=_side_stream())
    check_sort(hooks, rand_bits(rng, n, 64, np.uint64), rand_vals(rng, n), 39, stream=_side_stream())
    data = rand_vals(rng, 100_003)
    check_exclusive_sum(hooks, data, stream=_side_stream())
    check_suffix_min(hooks, data, stream=_side_stream())


@pytest.mark.gpu
def test_scratch_block_serves_different_sorts_uncleared(hooks):
    rng = np.random.default_rng(78)
    jobs = [(rand_bits(rng, 9 * 8192 + 1, 32, np.uint32), 27), (rand_bits(rng, 17 * 4096 + 100, 64, np.uint64), 39),
            (rand_bits(rng, 8193, 32, np.uint32), 32), (rand_bits(rng, 17 * 8192 + 100, 32, np.uint32), 9)]
    scratch = Scratch(max(query_sort_bytes(hooks, keys, keys.size, e) for keys, e in jobs))
    for keys, end_bit in jobs:
        check_sort(hooks, keys, rand_vals(rng, keys.size), end_bit, scratch=scratch)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [32, 64])
def test_sort_error_contract(hooks, width):
    rng = np.random.default_rng(79)
    n = TILE[width] + 1
    keys, vals = rand_bits(rng, n, width, KEY[width]), rand_vals(rng, n)
    r = run_sort(hooks, keys, vals, 27, short_by=1)  # one byte less than the size query asked for
    assert r.rc == HIP_ERROR_INVALID_VALUE
    assert r.ka.untouched() and r.kb.untouched() and r.va.untouched() and r.vb.untouched() and r.scratch.untouched()
    r = run_sort(hooks, keys, vals, 27, n_arg=0)       # nothing to sort: success, nothing written
    assert r.rc == HIP_SUCCESS
    assert r.ka.untouched() and r.kb.untouched() and r.va.untouched() and r.vb.untouched() and r.scratch.untouched()


# ---- the first pass's histogram from the caller ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("iota", [False, True])
@pytest.mark.parametrize("n", [8192, 9 * 8192 + 1, 17 * 8192 + 100])
@pytest.mark.parametrize("end_bit", [9, 10, 27, 28, 32])
def test_sort_u32_with_the_callers_histogram(hooks, end_bit, n, iota):
    """first_hist_ready: counts[digit * tiles + tile] of the first pass is in the scratch (computed here on the host from the RadixFirstPass
    fields) and the sort starts at its scatter.  Equal to the reference and to the sort that counts for itself."""
    rng = np.random.default_rng([32, n, end_bit, int(iota), 1])
    keys = rand_bits(rng, n, 32, np.uint32)
    vals = None if iota else rand_vals(rng, n)
    fused = check_sort(hooks, keys, vals, end_bit, hist=True)
    plain = check_sort(hooks, keys, vals, end_bit)
    assert np.array_equal(fused.keys, plain.keys) and np.array_equal(fused.vals, plain.vals)


# ---- the scans -------------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 2, 511, 512, 513, 4095, 4096, 4097, 100_003, 512 * 4096, 512 * 4096 + 1]  # (the last: a second round of scan_sums_kernel)


def run_scan(hooks, which, data, stream=None, short_by=0):
    n = data.size
    need = ctypes.c_size_t(0)
    if which == "sum":
        assert hooks.exclusive_sum_u32_u64(0, need, 0, 0, n) == HIP_SUCCESS
    else:
        assert hooks.suffix_min_u32(0, need, 0, n) == HIP_SUCCESS
    scratch, src = Scratch(need.value), Dev(data)
    out = Dev(np.full(n, UNWRITTEN[8], dtype=np.uint64)) if which == "sum" else src
    if stream is not None:
        _after_uploads(stream)
    handle = 0 if stream is None else stream.cuda_stream
    bytes_ = ctypes.c_size_t(need.value - short_by)
    if which == "sum":
        rc = hooks.exclusive_sum_u32_u64(scratch.ptr, bytes_, src.ptr, out.ptr, n, handle)
    else:
        rc = hooks.suffix_min_u32(scratch.ptr, bytes_, src.ptr, n, handle)
    _sync(stream)
    return types.SimpleNamespace(rc=rc, out=out.fetch(), src=src, dst=out, scratch=scratch)


def check_exclusive_sum(hooks, data, stream=None):
    r = run_scan(hooks, "sum", data, stream)
    assert r.rc == HIP_SUCCESS
    exp = np.zeros(data.size, dtype=np.uint64)
    exp[1:] = np.cumsum(data, dtype=np.uint64)[:-1]
    assert np.array_equal(r.out, exp)
    assert r.src.untouched()
    r.scratch.fetch()
    return exp


def check_suffix_min(hooks, data, stream=None):
    r = run_scan(hooks, "min", data, stream)
    assert r.rc == HIP_SUCCESS
    assert np.array_equal(r.out, np.minimum.accumulate(data[::-1])[::-1])
    r.scratch.fetch()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "past_2_33"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_sum(hooks, n, kind):
    rng = np.random.default_rng([1, n])
    data = rng.integers(0, 16, n, dtype=np.uint64).astype(np.uint32)
    if kind == "past_2_33":  # every seventh value near 2^32: the running sum passes 2^32 and 2^33 inside the array
        data[::7] = 0xFFFFFFFF - data[::7]
    exp = check_exclusive_sum(hooks, data)
    if kind == "past_2_33" and n >= 511:
        assert int(exp[-1]) > 2 ** 33


@pytest.mark.gpu
def test_exclusive_sum_refuses_a_short_scratch(hooks):
    r = run_scan(hooks, "sum", np.arange(4097, dtype=np.uint32), short_by=1)
    assert r.rc == HIP_ERROR_INVALID_VALUE and r.dst.untouched() and r.src.untouched() and r.scratch.untouched()
    r = run_scan(hooks, "min", np.arange(4097, dtype=np.uint32), short_by=1)
    assert r.rc == HIP_ERROR_INVALID_VALUE and r.src.untouched() and r.scratch.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "run_heads", "all_ones", "increasing", "decreasing"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_suffix_min(hooks, n, kind):
    rng = np.random.default_rng([2, n])
    if kind == "random":
        data = rand_vals(rng, n)
    elif kind == "run_heads":  # what the kNN directory hands it: 0xFFFFFFFF with the (increasing) run starts scattered in
        data = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        at = np.unique(rng.integers(0, max(n, 1), max(1, n // 700)))[:n]
        data[at] = np.sort(rng.integers(0, 1 << 31, at.size)).astype(np.uint32)
    elif kind == "all_ones":
        data = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    elif kind == "increasing":
        data = np.arange(n, dtype=np.uint32) + np.uint32(5)
    else:
        data = np.uint32(0xFFFFFFF0) - np.arange(n, dtype=np.uint32)
    check_suffix_min(hooks, data)


# ---- the products with the sort counting its own first histogram -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_products_pass_with_the_unfused_sort():
    """PST_SORT_FUSE=0: the key kernels of the voxel grid and of the kNN index count nothing and the sort runs its own histogram kernel for the
    first pass too.  The switch is read once per process, hence the child interpreter (one for both products)."""
    env = dict(os.environ, PST_SORT_FUSE="0")
    here = os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_voxel_grid.py"), os.path.join(here, "test_gpu_parity.py"), "-x", "-q", "-m", "gpu",
                        "-k", "test_random_cloud_matches_numpy or test_compute_normals_vs_oracle", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    passed = re.search(r"(\d+) passed", r.stdout)
    assert passed and int(passed.group(1)) >= 2 and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
