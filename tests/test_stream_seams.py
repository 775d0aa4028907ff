"""The fused Vec3f64 stream (pasture_amd/csrc/stream.hip, stream_tile.hpp) at every tile, phase and fold seam, against the numpy restatement of
tests/stream_ref.py.  Every comparison is on bits; nothing here has a tolerance.

The kernels count in 16-byte vectors, n_vec = (3 n - vec_first) / 2, and their tiles are 3 x 256 vectors (modes 2, 3), 3 x 512 (modes 6, 7) and
6 x 256 on a persistent grid (modes 4, 5); the point counts come from stream_ref.seam_counts, which turns vector counts at those seams into
points for both 16-byte phases, and test_launch_shape_steps_at_the_assumed_tiles fails first when the launch shape moves.  The launcher is called
directly (tests/cpp/stream_hooks.cpp forwards to pstk::launch_vec3f64_stream): ranges lie between sentinels, the scratch is exactly as large as
stream_partials_bytes says, poisoned with -inf / +inf records and followed by a canary, and the modes without a caller in the library (2: plain
copy, 5: read-only bounds of the transformed values) run like the others.  Planted extremes walk the (lane, row, half) classes of the rotated
accumulators; NaNs of every kind sit at the ragged head, in the body, in the partial tile and at the ragged tail; the record fold is called on
hand-made records on both sides of its two-level threshold.  The public entry points (convert_into_range, convert_into_with_bounds,
transform_attribute, calculate_bounds) run at the same seams, with the route each range pair takes asserted."""
import json
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import stream_hooks
import stream_ref as sr
from minmax_ref import F64_MAX, assert_same_aabb, assert_same_bits, bounds_ref
from pasture_amd.algorithms import calculate_bounds, transform_attribute
from pasture_amd.buffers import HashMapBuffer
from pasture_amd.conversion import BufferLayoutConverter, Transform, last_plan_kinds
from pasture_amd.layout import PointAttributeDataType as T, PointLayout, attributes as A
from stream_ref import SHAPE_READ, SHAPE_WRITE, SHAPE_WRITE_BOUNDS, n_vec_of, seam_counts, shape_of, stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

GUARD = 16                                  # sentinel doubles in front of and behind a range (even: the phase of a range is its `phase` alone)
SENTINEL = np.uint64(0x7FF4C0DEC0DE0000)    # (a signalling NaN: nothing computes it)
CANARY_BYTES = 1024
SCALE, OFFSET = (0.01, 0.001, 0.1), (-1234.5, 77.25, 0.125)
MODES = (2, 3, 4, 5, 6, 7)
BOUNDS_MODES = (4, 5, 6, 7)

QNAN_POS, QNAN_NEG = np.uint64(0x7FF8000000001234), np.uint64(0xFFF8000000FEDCBA)
SNAN_POS, SNAN_NEG = np.uint64(0x7FF0000000ABCDEF), np.uint64(0xFFF0000000123456)


def f64_bits(*values):
    return np.array(values, dtype=np.float64).view(np.uint64)


SPECIALS = np.concatenate([np.array([QNAN_POS, QNAN_NEG, SNAN_POS, SNAN_NEG], dtype=np.uint64), f64_bits(np.inf, -np.inf, 0.0, -0.0, F64_MAX, -F64_MAX)])


def random_bits(n_doubles, seed, lo=-1000.0, hi=1000.0):
    return np.random.default_rng(seed).uniform(lo, hi, n_doubles).view(np.uint64)


def count_with(shape, vec_first, n_vec):
    """the first point count of seam_counts(shape) with n_vec vectors at this phase, or with the nearest reachable count above"""
    pairs = seam_counts(*shape)[vec_first]
    return min((abs(v - n_vec), n) for n, v in pairs if v >= n_vec)[1]


def sweep_counts(shape, vec_first):
    return sorted(set(range(13)) | {n for n, _ in seam_counts(*shape)[vec_first]})


# ---- CPU: the helpers against plain arithmetic, the restatement against the oracle --------------------------------------------------------------
def vectors_by_hand(n_points, vec_first):
    """aligned pairs of doubles in a range of 3 n doubles that starts vec_first doubles behind a 16-byte boundary, counted one by one"""
    end = vec_first + 3 * n_points
    return sum(1 for a in range(vec_first, end) if a % 2 == 0 and a + 1 < end)


def test_seam_counts_yield_the_vectors_they_claim():
    assert [vectors_by_hand(n, f) for n, f in [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1)]] == [0, 0, 1, 1, 3, 2, 4]
    for shape in (SHAPE_WRITE, SHAPE_WRITE_BOUNDS, SHAPE_READ):
        tile, blk = shape
        counts = seam_counts(tile, blk)
        for vec_first in (0, 1):
            pairs = counts[vec_first]
            claimed = {v for _, v in pairs}
            for target in sr.seam_targets(tile, blk):  # every seam is hit, or bracketed by its nearest reachable neighbours
                assert target in claimed or (target - 1 in claimed and target + 1 in claimed) or (target == 0 and 1 in claimed), (shape, vec_first, target)
            assert all(n_vec_of(n, vec_first) == v for n, v in pairs)
            for n, v in pairs[:8] + pairs[len(pairs) // 2 - 2:len(pairs) // 2 + 2] + pairs[-2:]:  # a dozen of them, counted by hand
                assert vectors_by_hand(n, vec_first) == v, (shape, vec_first, n, v)
    # the seams of the three shapes in points, spelled out once
    assert dict(seam_counts(768, 256)[0])[512] == 768 and dict(seam_counts(768, 256)[1])[513] == 769
    assert dict(seam_counts(1536, 512)[0])[1024] == 1536 and dict(seam_counts(1536, 512)[0])[8193] == 8 * 1536 + 1
    assert count_with(SHAPE_READ, 0, 16 * 1536 + 1) == 16385


def oracle_positions(oracle, values):
    buf = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=oracle))
    buf.resize(values.shape[0])
    buf.set_attribute_range(A.POSITION_3D, range(0, values.shape[0]), values)
    return buf


def assert_same_but_nan_payloads(got_bits, want_bits, msg):
    got, want = np.asarray(got_bits).view(np.float64), np.asarray(want_bits).view(np.float64)
    assert got.shape == want.shape, msg
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{msg}: NaNs at {np.flatnonzero(np.isnan(got) != nan)[:8].tolist()}"
    bad = np.flatnonzero((np.asarray(got_bits) != np.asarray(want_bits)) & ~nan)
    assert bad.size == 0, f"{msg}: {bad.size} doubles differ, first at {bad[:8].tolist()}: got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"


def test_stream_ref_equals_the_oracle(oracle):
    """convert_into with Transform.affine on HashMapBuffers, then calculate_bounds: the reference of every comparison below, checked first."""
    rng = np.random.default_rng(11)
    for n, scale, offset in [(1, SCALE, OFFSET), (7, SCALE, OFFSET), (257, SCALE, OFFSET), (64, (0.0, 2.0, 1e10), (1.0, -1.0, 3.0)), (33, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))]:
        bits = rng.uniform(-1000.0, 1000.0, 3 * n).view(np.uint64)
        at = 3 + rng.permutation(3 * n - 3)[:2 * SPECIALS.size]  # (point 0 stays ordinary: calculate_bounds panics on a component of NaNs only)
        bits[at] = np.resize(SPECIALS, at.size)  # +-inf, NaNs, +-0 and +-MAX (MAX * 2 and MAX * 1e10 overflow, inf * 0 is a NaN)
        values = bits.view(np.float64).reshape(n, 3)
        src = oracle_positions(oracle, values)
        layout = src.point_layout()
        for mode in (6, 7):
            dst = HashMapBuffer.new_from_layout(layout)
            dst.resize(n)
            conv = BufferLayoutConverter.for_layouts(layout, layout)
            if mode & 1:
                conv.set_custom_mapping_with_transformation(A.POSITION_3D, A.POSITION_3D, Transform.affine(T.Vec3f64, scale, offset), False)
            conv.convert_into(src, dst)
            target, bounds = stream_ref(bits, n, scale, offset, mode)
            got = np.ascontiguousarray(dst.view_attribute(A.POSITION_3D)).reshape(-1).view(np.uint64)
            if mode & 1:
                assert_same_but_nan_payloads(got, target, f"n={n} mode={mode}")
            else:
                assert np.array_equal(got, target)
            assert_same_aabb(calculate_bounds(dst), bounds, f"n={n} mode={mode}")
            assert stream_ref(bits, n, scale, offset, mode & 5)[0] is None and stream_ref(bits, n, scale, offset, mode & 3)[1] is None
            assert_same_bits(np.concatenate(stream_ref(bits, n, scale, offset, mode & 5)[1]), np.concatenate(bounds))
    mn, mx = stream_ref(np.zeros(0, dtype=np.uint64), 0, SCALE, OFFSET, 7)[1]
    assert mn.tolist() == [F64_MAX] * 3 and mx.tolist() == [-F64_MAX] * 3
    eps = 2.0 ** -52  # (1 + eps)^2 = 1 + 2 eps + eps^2 rounds to 1 + 2 eps before the offset is added; an fma would keep the eps^2
    two = stream_ref(f64_bits(1.0 + eps, 1.0, 1.0), 1, (1.0 + eps, 1.0, 1.0), (-1.0, 0.0, 0.0), 3)[0].view(np.float64)
    assert two.tolist() == [2.0 * eps, 1.0, 1.0]


# ---- GPU: the launcher, called directly ----------------------------------------------------------------------------------------------------------
class Device:
    """torch, the hooks and the small shared device state of the direct calls"""

    def __init__(self):
        import torch
        self.torch = torch
        self.hooks = stream_hooks.load()  # (raises "run build()" when the library is missing: never a skip)
        self.dev = torch.device("cuda")
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.out6 = torch.empty(6, dtype=torch.float64, device=self.dev)
        self.sentinel = int(SENTINEL.view(np.int64))

    def upload(self, bits):
        return self.torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(self.dev)

    def poisoned_records(self, n_records):
        """n_records records of {-inf x 3, +inf x 3}: a stale record that wins every fold it enters"""
        t = self.torch.empty((n_records, 6), dtype=self.torch.float64, device=self.dev)
        t[:, :3] = -np.inf
        t[:, 3:] = np.inf
        return t.reshape(-1)

    def stream_handle(self):
        return self.torch.cuda.current_stream().cuda_stream

    def sync(self):
        self.torch.cuda.current_stream().synchronize()


@pytest.fixture(scope="module")
def device(hip):
    return Device()


class Master:
    """A range of doubles on the host and on the device, `phase` doubles behind a 16-byte boundary, with GUARD doubles of other data around it; a
    second device copy tells whether a call wrote to its source."""

    def __init__(self, device, range_bits, phase, seed=99):
        self.device, self.phase, self.lo = device, phase, GUARD + phase
        self.host = np.concatenate([random_bits(self.lo, seed), np.ascontiguousarray(range_bits, dtype=np.uint64), random_bits(GUARD + 2, seed + 1)])
        self.dev = device.upload(self.host)
        self.pristine = self.dev.clone()
        assert self.dev.data_ptr() % 16 == 0 and self.pristine.data_ptr() % 16 == 0
        self.capacity = (len(range_bits)) // 3

    @contextmanager
    def patched(self, edits):
        """{index of a double in the range: bits}, on the host and on the device, undone afterwards"""
        torch = self.device.torch
        idx = np.fromiter(edits.keys(), dtype=np.int64) + self.lo
        new = np.array([np.uint64(v) for v in edits.values()], dtype=np.uint64)
        old = self.host[idx].copy()
        where = torch.from_numpy(idx).to(self.device.dev)

        def put(bits):
            self.host[idx] = bits
            on_device = self.device.upload(bits)
            self.dev[where] = on_device
            self.pristine[where] = on_device
        put(new)
        try:
            yield self
        finally:
            put(old)


def check_bounds(got6, want, msg, negated=False, zeros_by_value=False):
    want6 = np.concatenate(want).astype(np.float64)
    if negated:
        want6[3:] = -want6[3:]
    got6 = np.asarray(got6, dtype=np.float64)
    if zeros_by_value:  # mode 5 (kernels.hpp): a +-0 bound has no defined sign
        keep = want6 != 0
        assert np.array_equal(got6[~keep], want6[~keep]), f"{msg}: got {got6.tolist()} want {want6.tolist()}"
        got6, want6 = got6[keep], want6[keep]
    assert_same_bits(got6, want6, msg)


def run_case(device, master, n, mode, scale=SCALE, offset=OFFSET, in_place=False, loose_nans=False, negated=False, check_target=True, want=None):
    """One launch of the first n points of `master` through the hooks, everything around it checked: the target bits, the sentinels on both sides
    of the target, the source, the bounds, the unused part of the scratch and the canary behind it.  want: stream_ref's answer when the caller
    has it already."""
    torch, hooks = device.torch, device.hooks
    lo, hi = master.lo, master.lo + 3 * n
    assert n <= master.capacity
    msg = f"mode={mode} phase={master.phase} n={n} n_vec={n_vec_of(n, master.phase)}{' in place' if in_place else ''}"
    target, bounds = want if want is not None else stream_ref(master.host[lo:hi], n, scale, offset, mode)
    write = bool(mode & 2)
    assert not in_place or write

    if in_place:
        arena = master.dev[:hi + GUARD].clone()
        arena[lo - GUARD:lo] = device.sentinel
        arena[hi:] = device.sentinel
        expected = master.host[:hi + GUARD].copy()
        expected[lo - GUARD:lo] = SENTINEL
        expected[hi:] = SENTINEL
        src = arena
    else:
        size = hi + GUARD if write else 0  # (a mode that does not write is given no target)
        arena = torch.full((size,), device.sentinel, dtype=torch.int64, device=device.dev)
        expected = np.full(size, SENTINEL, dtype=np.uint64)
        src = master.dev
    if write:
        expected[lo:hi] = target
    assert arena.data_ptr() % 16 == 0

    # the scratch: exactly stream_partials_bytes, every record poisoned, then the canary (and as many poisoned records again as the launch has,
    # checked like the canary)
    nbytes = hooks.partials_bytes(n, mode)
    assert nbytes % 48 == 0
    records = nbytes // 48
    canary_doubles = CANARY_BYTES // 8 + records * 6
    scratch = torch.cat([device.poisoned_records(records), device.poisoned_records((canary_doubles + 5) // 6)])
    before = scratch.clone()
    device.out6.fill_(12345.0)
    if negated:
        hooks.set_record_form(device.out6.data_ptr(), 1)
    try:
        hooks.launch(src.data_ptr() + 8 * lo, arena.data_ptr() + 8 * lo if write else 0, n, scale if mode & 1 else None, offset if mode & 1 else None, mode,
                     scratch.data_ptr(), device.out6.data_ptr(), device.stream_handle())
        device.sync()
    finally:
        if negated:
            hooks.set_record_form(device.out6.data_ptr(), 0)

    if check_target and write:
        got = arena.cpu().numpy().view(np.uint64)
        if loose_nans:
            assert np.array_equal(got[:lo], expected[:lo]) and np.array_equal(got[hi:], expected[hi:]), f"{msg}: a double outside the target range changed"
            assert_same_but_nan_payloads(got[lo:hi], expected[lo:hi], msg)
        elif not np.array_equal(got, expected):
            bad = np.flatnonzero(got != expected)
            where = ["in front of the range" if i < lo else "behind the range" if i >= hi else f"double {i - lo} = point {(i - lo) // 3}" for i in bad[:6]]
            raise AssertionError(f"{msg}: {bad.size} doubles differ: {where}; got {[hex(int(x)) for x in got[bad[:4]]]} want {[hex(int(x)) for x in expected[bad[:4]]]}")
    assert torch.equal(master.dev[:hi + GUARD], master.pristine[:hi + GUARD]), f"{msg}: the source changed"
    out6 = device.out6.cpu().numpy()
    if mode & 4:
        check_bounds(out6, bounds, msg, negated=negated, zeros_by_value=(mode & 7) == 5)
    else:
        assert out6.tolist() == [12345.0] * 6, f"{msg}: a mode without bounds wrote the record"
    blocks = records - sr.FOLD_BLOCKS  # (the room for first-level records behind them is used above the fold's threshold only)
    used = 0 if not mode & 4 else records * 6 if blocks > sr.FOLD_TWO_LEVEL_ABOVE else blocks * 6
    assert torch.equal(scratch[used:].view(torch.int64), before[used:].view(torch.int64)), f"{msg}: the scratch behind stream_partials_bytes changed"


def expected_blocks(n_points, mode, cus):
    tile = shape_of(mode)[0]
    tiles = max(1, -(-((3 * n_points) // 2) // tile))
    return 8 * -(-tiles // 8) if mode & 2 else min(tiles, 4 * cus)


@gpu
def test_launch_shape_steps_at_the_assumed_tiles(device):
    """Blocks of a launch = stream_partials_bytes / 48 - 128 (kFoldBlocks).  Whoever changes the launch shape fails here first: SHAPE_* of
    tests/stream_ref.py, and with them every seam below, follow stream_shape() and kStreamLoads."""
    for mode in MODES:
        tile_points = shape_of(mode)[0] * 2 // 3
        counts = list(range(0, 17 * tile_points + 3)) + [k * tile_points + d for k in (4 * device.cus - 1, 4 * device.cus, 4 * device.cus + 1, 4096, 4097) for d in (-1, 0, 1)]
        for n in counts:
            nbytes = device.hooks.partials_bytes(n, mode)
            assert nbytes % 48 == 0 and nbytes // 48 - sr.FOLD_BLOCKS == expected_blocks(n, mode, device.cus), (mode, n, nbytes)


@pytest.fixture(scope="module")
def sweep_masters(device):
    """per phase: random values, and values of {+0, -0, 1.5, 2.5} (a zero bound at every count, its sign that of the first zero)"""
    n_max = max(n for shape in (SHAPE_WRITE, SHAPE_WRITE_BOUNDS, SHAPE_READ) for f in (0, 1) for n, _ in seam_counts(*shape)[f])
    zeros = np.random.default_rng(5).choice(f64_bits(0.0, -0.0, 1.5, 2.5), 3 * n_max)
    return {phase: (Master(device, random_bits(3 * n_max, 1 + phase), phase), Master(device, zeros, phase)) for phase in (0, 1)}


@gpu
@pytest.mark.parametrize("mode,in_place", [(m, False) for m in MODES] + [(3, True), (7, True)])
def test_every_seam_count_at_both_phases(device, sweep_masters, mode, in_place):
    for phase in (0, 1):
        random_master, zeros_master = sweep_masters[phase]
        for n in sweep_counts(shape_of(mode), phase):
            run_case(device, random_master, n, mode, in_place=in_place)
            run_case(device, zeros_master, n, mode, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), in_place=in_place)


@gpu
def test_nothing_written_for_no_points(device, sweep_masters):
    for mode in MODES:
        for phase in (0, 1):
            run_case(device, sweep_masters[phase][0], 0, mode, want=(np.zeros(0, dtype=np.uint64) if mode & 2 else None, sr.seeds() if mode & 4 else None))


@gpu
@pytest.mark.parametrize("mode", BOUNDS_MODES)
def test_poisoned_scratch_with_surplus_blocks(device, sweep_masters, mode):
    """8 tiles + 1 vector: a grid of 16 with 7 surplus blocks, whose records must be identities, not what an earlier call left there (run_case
    poisons the scratch of every call in this file; the count that takes the two-level fold, 4097 tiles, is
    test_write_modes_on_both_sides_of_the_two_level_fold)."""
    tile = shape_of(mode)[0]
    for phase in (0, 1):
        n = count_with(shape_of(mode), phase, 8 * tile + 1)
        assert n_vec_of(n, phase) in (8 * tile + 1, 8 * tile + 2)
        blocks = device.hooks.partials_bytes(n, mode) // 48 - sr.FOLD_BLOCKS
        assert blocks == (16 if mode & 2 else 9)
        run_case(device, sweep_masters[phase][0], n, mode)


def class_points(shape, vec_first, n):
    """the points of a range of n that hold the doubles of lanes {0, 1, 2, 63, 64, BLK - 1} in every row of the first and of the last (partial)
    tile, the points on either side of every tile boundary, and the first and the last point"""
    tile, blk = shape
    n_vec = n_vec_of(n, vec_first)
    points = {0, n - 1}
    for t in (0, (n_vec - 1) // tile):
        for lane in (0, 1, 2, 63, 64, blk - 1):
            points |= {d // 3 for d, _, _ in sr.lane_doubles(shape, vec_first, t, lane) if (d - vec_first) // 2 < n_vec}
    for t in range(1, (n_vec + tile - 1) // tile):
        boundary = vec_first + 2 * t * tile  # first double of tile t
        points |= {(boundary - 1) // 3, boundary // 3, (boundary - 1) // 3 - 1, boundary // 3 + 1}
    return sorted(p for p in points if 0 <= p < n)


def extremes(i, other, sign=1.0):
    """point i = (-3, 3, -3), point `other` = (3, -3, 3): every bound is +-3 and has exactly one point that holds it"""
    lo, hi = f64_bits(-3.0 * sign, 3.0 * sign, -3.0 * sign), f64_bits(3.0 * sign, -3.0 * sign, 3.0 * sign)
    return {**{3 * i + c: lo[c] for c in range(3)}, **{3 * other + c: hi[c] for c in range(3)}}


@gpu
@pytest.mark.parametrize("mode", (4, 6, 7))
def test_planted_extremes_in_every_lane_row_and_half_class(device, mode):
    """Random data checks one (lane, row, half) class per run; a wrong rotation of the accumulators shows only when the extreme of a component
    sits in the class it gets wrong."""
    shape = shape_of(mode)
    n = 2 * (shape[0] * 2 // 3) + 5
    for phase in (0, 1):
        master = Master(device, random_bits(3 * n, 40 + phase, 1.0, 2.0), phase)
        points = class_points(shape, phase, n)
        assert len(points) >= 5 * sr.rows_of(shape)  # (per row of tile 0: lanes 0..2, lanes 63 and 64, the last lane)
        for i in points:
            for sign in (1.0, -1.0):
                with master.patched(extremes(i, (i + n // 2 + 1) % n, sign)):
                    run_case(device, master, n, mode)


@gpu
def test_mode_4_past_the_persistent_grid(device):
    """More tiles than the 4 blocks per CU of the persistent grid: the grid-stride loop wraps, and the extremes sit in the first tile of the
    second sweep and in the last, partial, tile."""
    grid = 4 * device.cus
    n = 1024 * grid + 1025
    assert device.hooks.partials_bytes(n, 4) // 48 - sr.FOLD_BLOCKS == grid
    for phase in (0, 1):
        master = Master(device, random_bits(3 * n, 50 + phase, 1.0, 2.0), phase)
        run_case(device, master, n, 4)
        for i, other in [(1024 * grid + 3, n - 1), (n - 1, 1024 * grid + 700), (1024 * grid - 1, 1024 * grid)]:
            with master.patched(extremes(i, other)):
                mn, mx = sr.seeds()
                mn[:], mx[:] = -3.0, 3.0
                run_case(device, master, n, 4, want=(None, (mn, mx)))
                run_case(device, master, n, 5, scale=(2.0, 1.0, 0.5), offset=(1.0, 0.0, -1.0), want=(None, (np.array([-5.0, -3.0, -2.5]), np.array([7.0, 3.0, 0.5]))))


class Big:
    """4097 tiles of the 1024-point shapes, about 100 MB, shared by the cases on either side of the two-level fold; answers are kept per (mode, n)"""

    def __init__(self, device):
        self.n = 4097 * 1024
        self.master = Master(device, random_bits(3 * self.n, 60), 0)
        self.answers = {}

    def want(self, mode, n):
        if (mode, n) not in self.answers:
            self.answers[(mode, n)] = stream_ref(self.master.host[self.master.lo:self.master.lo + 3 * n], n, SCALE, OFFSET, mode)
        return self.answers[(mode, n)]


@pytest.fixture(scope="module")
def big(device):
    return Big(device)


@gpu
@pytest.mark.parametrize("n_records", [1, 2, 255, 256, 257, 4095, 4096, 4097, 4104, 4224, 4225])
def test_record_fold_on_both_sides_of_its_threshold(device, n_records):
    """launch_finalize_bounds on hand-made records: one level up to 4096 records, above that 128 first-level records written at
    partials + n_records * 6 (the scratch contract of bounds_partials_bytes) and a second level over exactly those."""
    torch, hooks = device.torch, device.hooks
    assert hooks.bounds_partials_bytes(n_records) == (n_records + sr.FOLD_BLOCKS) * 48
    gen = torch.Generator(device="cpu").manual_seed(n_records)
    for where in (0, n_records - 1):
        records = 1.0 + torch.rand((n_records, 6), dtype=torch.float64, generator=gen)
        records[:, 3:] *= -1.0  # minima in [1, 2), maxima in (-2, -1]: only the planted record holds a bound
        records[where] = torch.tensor([-5.0, -6.0, -7.0, 5.0, 6.0, 7.0], dtype=torch.float64)
        room = device.poisoned_records(sr.FOLD_BLOCKS + n_records + 22)  # the first-level room, then the canary
        scratch = torch.cat([records.to(device.dev).reshape(-1), room])
        before = scratch.clone()
        for negated in (False, True):
            device.out6.fill_(12345.0)
            hooks.set_record_form(device.out6.data_ptr(), 1 if negated else 0)
            try:
                hooks.finalize_bounds(scratch.data_ptr(), n_records, device.out6.data_ptr(), device.stream_handle())
                device.sync()
            finally:
                hooks.set_record_form(device.out6.data_ptr(), 0)
            sign = -1.0 if negated else 1.0
            assert device.out6.cpu().tolist() == [-5.0, -6.0, -7.0, sign * 5.0, sign * 6.0, sign * 7.0], (n_records, where, negated)
            keep = n_records * 6
            assert torch.equal(scratch[:keep], before[:keep]), "the fold changed its records"
            behind = (n_records + sr.FOLD_BLOCKS) * 6
            assert torch.equal(scratch[behind:], before[behind:]), "the fold wrote behind bounds_partials_bytes"
            if n_records <= sr.FOLD_TWO_LEVEL_ABOVE:
                assert torch.equal(scratch[keep:], before[keep:]), "a one-level fold wrote first-level records"


@gpu
@pytest.mark.parametrize("mode", (6, 7))
@pytest.mark.parametrize("tiles", (4096, 4097))
def test_write_modes_on_both_sides_of_the_two_level_fold(device, big, mode, tiles):
    n = tiles * 1024
    records = device.hooks.partials_bytes(n, mode) // 48 - sr.FOLD_BLOCKS
    assert records == (4096 if tiles == 4096 else 4104) and (records > sr.FOLD_TWO_LEVEL_ABOVE) == (tiles == 4097)
    run_case(device, big.master, n, mode, want=big.want(mode, n))


@gpu
def test_record_form_min_and_negated_max(device, sweep_masters, big):
    """pst_bounds_record_set_form: the last fold kernel writes {min, -max}, on one fold level and on two"""
    for mode in (4, 6, 7):
        for phase in (0, 1):
            for n in (1, 5, count_with(shape_of(mode), phase, shape_of(mode)[0] + 1)):
                run_case(device, sweep_masters[phase][0], n, mode, negated=True)
                run_case(device, sweep_masters[phase][1], n, mode, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), negated=True)
    for mode in (6, 7):
        n = 4097 * 1024
        run_case(device, big.master, n, mode, negated=True, check_target=False, want=big.want(mode, n))
    run_case(device, sweep_masters[0][0], 7, 6)  # and the form is off again


def with_specials(n, phase, shape, rotation, seed):
    """random values in [1, 2) with SPECIALS at the ragged head, in the body, in the partial tile and at the ragged tail of the range"""
    bits = random_bits(3 * n, seed, 1.0, 2.0)
    last_tile = phase + 2 * ((n_vec_of(n, phase) - 1) // shape[0]) * shape[0]
    at = [0, 1, 2, 3, 129, 130, 2 * shape[1] + 1, 2 * shape[1] + 2, last_tile - 1, last_tile, last_tile + 1, last_tile + 4, 3 * n - 3, 3 * n - 2, 3 * n - 1]
    for k, d in enumerate(at):
        bits[d] = SPECIALS[(k + rotation) % SPECIALS.size]
    return bits


@gpu
@pytest.mark.parametrize("mode", (2, 3, 4, 5, 6, 7))
def test_nans_infinities_and_zeros_at_head_body_partial_tile_and_tail(device, mode):
    """The copy modes keep every bit, signalling NaNs included; the affine modes match numpy in NaN-ness and in every bit that is not a NaN's
    (inf * 0 and MAX * 2 among them); the bounds ignore every NaN."""
    shape = shape_of(mode)
    base = 2 * (shape[0] * 2 // 3) + 5
    for phase in (0, 1):
        for n in (base, base + 1):  # (one of them has a ragged tail at this phase)
            for rotation in range(SPECIALS.size):
                master = Master(device, with_specials(n, phase, shape, rotation, 70 + rotation), phase)
                run_case(device, master, n, mode, scale=(0.0, 2.0, 0.5), offset=(1.0, -1.0, 3.0), loose_nans=bool(mode & 1))
                if mode & 2:
                    run_case(device, master, n, mode, scale=(0.0, 2.0, 0.5), offset=(1.0, -1.0, 3.0), loose_nans=bool(mode & 1), in_place=True)
    assert {n_vec_of(n, f) * 2 + f < 3 * n for n in (base, base + 1) for f in (0, 1)} == {True, False}


@gpu
@pytest.mark.parametrize("mode", BOUNDS_MODES)
def test_a_component_of_nans_only_leaves_its_seeds(device, mode):
    shape = shape_of(mode)
    for phase in (0, 1):
        for n in (1, 2, 9, shape[0] * 2 // 3 + 7):
            for comp in range(3):
                bits = random_bits(3 * n, 80 + comp, -2.0, 2.0)
                bits[comp::3] = np.resize(np.array([QNAN_POS, SNAN_POS, QNAN_NEG, SNAN_NEG], dtype=np.uint64), n)
                want = stream_ref(bits, n, SCALE, OFFSET, mode)
                assert want[1][0][comp] == F64_MAX and want[1][1][comp] == -F64_MAX
                run_case(device, Master(device, bits, phase), n, mode, loose_nans=bool(mode & 1), want=want)


@gpu
@pytest.mark.parametrize("mode", (4, 6))
def test_a_signalling_nan_does_not_cost_a_lane_its_extreme(device, mode):
    """A raw v_min_f64 / v_max_f64 returns a quieted NaN for a signalling operand, and the next fold would then drop the accumulator: the lane's
    earlier extreme is lost.  The only holder of a bound and a signalling NaN share one accumulator (same lane, same component), the NaN as the
    first and as the last value folded into it; likewise the ragged head and tail doubles, which lanes 0 and 1 of block 0 fold last."""
    shape = shape_of(mode)
    n = 2 * (shape[0] * 2 // 3) + 5
    for phase in (0, 1):
        master = Master(device, random_bits(3 * n, 90 + phase, 1.0, 2.0), phase)
        cases = []
        for tile, lane in [(0, 0), (0, 1), (0, 5), (0, 70), (1, 3), (1, shape[1] - 1)]:
            shared = {}  # doubles by accumulator: the rotated component in stream_tile.hpp, (row mod 3, half) in stream.hip
            for d, j, h in sr.lane_doubles(shape, phase, tile, lane):
                shared.setdefault(d % 3 if mode & 2 else (j % 3, h), []).append(d)
            for same in shared.values():
                assert len(same) == 2 and same[0] % 3 == same[1] % 3
                cases += [(same[0], same[1]), (same[1], same[0])]
        assert len(cases) == 6 * 2 * (3 if mode & 2 else 6)
        n_vec = n_vec_of(n, phase)
        if phase == 1:  # the head double (x of point 0), folded by lane 0 of block 0 behind its own doubles
            cases += [(0, d) for d, _, _ in sr.lane_doubles(shape, phase, 0, 0) if d % 3 == 0][:1]
        if phase + 2 * n_vec < 3 * n:  # the tail double, folded by lane 1 of block 0
            tail = 3 * n - 1
            cases += [(tail, d) for d, _, _ in sr.lane_doubles(shape, phase, 0, 1) if d % 3 == tail % 3][:1]
        for nan_at, extreme_at in cases:
            for nan in (SNAN_POS, SNAN_NEG):
                for value in (-3.0, 3.0):
                    with master.patched({nan_at: nan, extreme_at: f64_bits(value)[0]}):
                        run_case(device, master, n, mode)
    # (n + 1 has its ragged tail at the other phase)
    for phase in (0, 1):
        m = n + 1
        if phase + 2 * n_vec_of(m, phase) < 3 * m:
            master = Master(device, random_bits(3 * m, 95, 1.0, 2.0), phase)
            tail = 3 * m - 1
            extreme_at = [d for d, _, _ in sr.lane_doubles(shape, phase, 0, 1) if d % 3 == tail % 3][0]
            for value in (-3.0, 3.0):
                with master.patched({tail: SNAN_POS, extreme_at: f64_bits(value)[0]}):
                    run_case(device, master, m, mode)


@gpu
def test_on_a_side_stream(device, sweep_masters):
    torch = device.torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for mode in MODES:
        n = count_with(shape_of(mode), 1, 2 * shape_of(mode)[0] + 1)
        with torch.cuda.stream(side):
            assert device.stream_handle() == side.cuda_stream != 0
            run_case(device, sweep_masters[1][0], n, mode)  # (run_case reads its results after stream.synchronize() of the current stream)
    torch.cuda.current_stream().wait_stream(side)


# ---- GPU: through the public API ------------------------------------------------------------------------------------------------------------------
API_COUNTS = sorted({count_with(shape, 0, 8 * shape[0] + 1) for shape in (SHAPE_WRITE, SHAPE_WRITE_BOUNDS, SHAPE_READ)})


def columnar(api, values):
    buf = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=api))
    buf.resize(values.shape[0])
    buf.set_attribute_range(A.POSITION_3D, range(0, values.shape[0]), values)
    return buf


def position_bits(buf):
    return np.ascontiguousarray(buf.view_attribute(A.POSITION_3D)).reshape(-1).view(np.uint64)


@gpu
@pytest.mark.parametrize("s0,t0", [(0, 0), (1, 1), (2, 0), (1, 0), (0, 1), (3, 2)])
def test_range_pairs_take_the_stream_only_in_the_same_phase(hip, s0, t0):
    """converter.cpp takes the stream when source and target range share their 16-byte phase (s0 - t0 even); every other pair takes the column
    kernels, and is as right."""
    assert API_COUNTS == [4097, 8193]
    for n in API_COUNTS:
        total = n + 5
        rng = np.random.default_rng(n + s0)
        src_values, old_values = rng.uniform(-1000.0, 1000.0, (total, 3)), rng.uniform(-1.0, 1.0, (total, 3))
        src = columnar(hip, src_values)
        layout = src.point_layout()
        src_bits = src_values.reshape(-1).view(np.uint64)[3 * s0:3 * (s0 + n)]
        for affine in (True, False):
            conv = BufferLayoutConverter.for_layouts(layout, layout)
            if affine:
                conv.set_custom_mapping_with_transformation(A.POSITION_3D, A.POSITION_3D, Transform.affine(T.Vec3f64, SCALE, OFFSET), False)
            target, bounds = stream_ref(src_bits, n, SCALE, OFFSET, 7 if affine else 6)
            expected = old_values.reshape(-1).view(np.uint64).copy()
            expected[3 * t0:3 * (t0 + n)] = target
            for with_bounds in ((False, True) if affine else (True,)):
                dst = columnar(hip, old_values)
                if with_bounds:
                    got = conv.convert_into_with_bounds(src, dst, range(s0, s0 + n), range(t0, t0 + n))
                else:
                    conv.convert_into_range(src, range(s0, s0 + n), dst, range(t0, t0 + n))
                msg = f"n={n} s0={s0} t0={t0} affine={affine} bounds={with_bounds}"
                assert ("stream" in last_plan_kinds(hip)) == ((s0 - t0) % 2 == 0), (msg, last_plan_kinds(hip))
                assert np.array_equal(position_bits(dst), expected), msg  # the range, and the previous bits around it
                assert np.array_equal(position_bits(src), src_values.reshape(-1).view(np.uint64)), msg
                if with_bounds:
                    assert_same_aabb(got, bounds, msg)
                    assert_same_aabb(got, bounds_ref(target.view(np.float64).reshape(n, 3)), msg)


@gpu
def test_transform_attribute_and_bounds_of_an_odd_slice(hip):
    for n in API_COUNTS:
        values = np.random.default_rng(n).uniform(-1000.0, 1000.0, (n, 3))
        buf = columnar(hip, values)
        bits = values.reshape(-1).view(np.uint64)
        for first in (1, 3, 2):
            assert_same_aabb(calculate_bounds(buf.slice(range(first, n))), bounds_ref(values[first:]), f"slice from {first} of {n}")
        transform_attribute(buf, A.POSITION_3D, Transform.affine(T.Vec3f64, SCALE, OFFSET))
        target, bounds = stream_ref(bits, n, SCALE, OFFSET, 7)
        assert np.array_equal(position_bits(buf), target), n
        assert_same_aabb(calculate_bounds(buf), bounds, f"n={n}")
        transform_attribute(buf.slice(range(1, n)), A.POSITION_3D, Transform.affine(T.Vec3f64, SCALE, OFFSET))  # in place, 8 bytes off
        again = stream_ref(target[3:], n - 1, SCALE, OFFSET, 3)[0]
        assert np.array_equal(position_bits(buf), np.concatenate([target[:3], again])), n


# ---- GPU: the switches, each in a fresh child process (they are read once per process) -----------------------------------------------------------
def switch_child():
    """modes 3, 6, 7 at 8 tiles + 1 vector (7 surplus blocks, XCD-aware or plain numbering), both phases"""
    device = Device()
    out = {"cases": 0, "failures": []}
    for mode in (3, 6, 7):
        shape = shape_of(mode)
        for phase in (0, 1):
            n = count_with(shape, phase, 8 * shape[0] + 1)
            master = Master(device, random_bits(3 * n, 7 * mode + phase), phase)
            try:
                run_case(device, master, n, mode)
                run_case(device, master, n, mode, in_place=True)
            except AssertionError as e:
                out["failures"].append(str(e)[:400])
            out["cases"] += 1
    return out


@gpu
@pytest.mark.parametrize("switch,value", [("PST_STREAM_XCD", "0"), ("PST_STREAM_RESIDENT", "1"), ("PST_STREAM_RESIDENT", "8")])
def test_switches_in_a_child_process(hip, switch, value):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), **{switch: value})
    script = "import json\nimport test_stream_seams as t\nprint('RESULT ' + json.dumps(t.switch_child()))\n"
    child = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stdout + child.stderr
    result = json.loads([line for line in child.stdout.splitlines() if line.startswith("RESULT ")][-1][len("RESULT "):])
    assert result == {"cases": 6, "failures": []}, result
