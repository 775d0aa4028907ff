"""The compaction of pasture_amd/csrc/filter.hip and filter_stream.hpp at its seams, against the numpy reference of tests/filter_ref.py.  Every
comparison is exact.

Count and scan are called directly (tests/cpp/filter_hooks.cpp forwards to pstk::launch_filter_count): the count kernel's switch between four whole
tiles per wave and the vector loop with a byte tail (every 8192 points), every byte value as "selected" (the contract is mask[i] != 0), masks at
odd addresses; the many-block scan at 1024 / 1025 tiles, at its block borders and at 2^19 tiles, the one-block scan at its rounds of 4096 tiles
and its look-ahead of 32 768.  The compaction itself runs through the public API with masks whose tiles hold exactly cap - 1, cap, cap + 1, 2 cap,
2 cap + 1 ... matches, cap being the points of one LDS round of the layout's kernel -- sizes a random mask never produces."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import filter_hooks
import filter_ref as fr
from filter_ref import HOSTILE, TILE
from harness import custom_point_type_big, random_records
from pasture_amd import conversion as cv
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition, PointLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256          # bytes before and behind the workspace (keeps its alignment)
FILL = 0xA5          # what the workspace holds before a call (the product reuses its scratch uncleared)
UNWRITTEN = 0xAB     # what a target holds before a compaction


@pytest.fixture(scope="module")
def hooks():
    return filter_hooks.load()  # (raises "run build()" when the library is missing: never a skip)


@pytest.fixture
def jit_sync(hip):
    cv.jit_set_mode("sync", api=hip)
    yield
    cv.jit_set_mode("env", api=hip)


# ---- CPU: the reference against plain loops -----------------------------------------------------------------------------------------------------
def test_reference_against_plain_loops():
    rng = np.random.default_rng(7)
    every = np.arange(256, dtype=np.uint8)  # all 256 byte values: exactly one of them is "not selected"
    assert int(fr.tile_counts(every, tile=256)[0]) == 255 and fr.tile_counts(every, tile=100).tolist() == [99, 100, 56]
    for n, tile in [(0, 16), (1, 16), (15, 16), (16, 16), (17, 16), (300, 16), (256, 100), (777, 2048)]:
        mask = rng.permutation(np.resize(every, n)).astype(np.uint8)
        mask[rng.random(n) < 0.5] = 0
        counts = [sum(1 for b in mask[t:t + tile] if b != 0) for t in range(0, n, tile)]
        got = fr.tile_counts(mask, tile)
        assert got.dtype == np.uint32 and got.tolist() == counts, (n, tile)
        offsets, run = [], 0
        for c in counts:
            offsets.append(run)
            run += c
        offsets.append(run)
        got = fr.tile_offsets(got)
        assert got.dtype == np.uint64 and got.tolist() == offsets, (n, tile)
        rec = np.zeros(n, dtype=[("a", np.uint16), ("b", np.float64, (3,))])
        rec["a"] = np.arange(n)
        rec["b"] = rng.random((n, 3))
        keep = [i for i in range(n) if mask[i] != 0]
        assert fr.compact(rec, mask)["a"].tolist() == keep and fr.compact(rec, mask).tobytes() == b"".join(rec[i].tobytes() for i in keep)
        for limit in (0, 1, len(keep) // 2, len(keep), len(keep) + 3):
            assert fr.compact_limited(rec, mask, limit)["a"].tolist() == keep[:limit]
    assert fr.tile_offsets(np.full(3, 0xFFFFFFFF, dtype=np.uint32)).tolist() == [0, 0xFFFFFFFF, 2 * 0xFFFFFFFF, 3 * 0xFFFFFFFF]  # (no 32-bit wrap)


def test_mask_builders_place_what_they_say():
    counts = [5, 0, 16, 1, 16, 15]
    for kind in fr.POSITIONS:
        mask = fr.mask_with_counts(counts, 7, np.random.default_rng(1), HOSTILE, kind, tail_count=3, tile=16)
        assert mask.dtype == np.uint8 and mask.size == 6 * 16 + 7
        assert fr.tile_counts(mask, 16).tolist() == counts + [3], kind
        assert set(np.unique(mask).tolist()) <= set(HOSTILE) | {0}
        at = np.flatnonzero(mask[:16]).tolist()
        if kind != "random":
            assert {"first": at == [0, 1, 2, 3, 4], "last": at == [11, 12, 13, 14, 15], "first_and_last": at == [0, 1, 2, 14, 15],
                    "run": at == list(range(at[0], at[0] + 5))}[kind], (kind, at)
        assert np.array_equal(mask, fr.mask_with_counts(counts, 7, np.random.default_rng(1), HOSTILE, kind, tail_count=3, tile=16))  # deterministic
    mixed = fr.mask_with_counts([1, 1, 3], 0, None, (0x80,), ["first", "last", "random"], tile=16)
    assert mixed[0] == 0x80 and mixed[31] == 0x80 and fr.tile_counts(mixed, 16).tolist() == [1, 1, 3] and set(np.unique(mixed).tolist()) == {0, 0x80}
    many = fr.mask_with_counts(np.arange(3000) % 2049, 5, None, HOSTILE, "run")
    assert np.array_equal(fr.tile_counts(many), np.append(np.arange(3000) % 2049, 0).astype(np.uint32))
    with pytest.raises(ValueError):
        fr.mask_with_counts([17], tile=16)


def stream_cap_for(total):
    """filter.hip's stream_cap_for, restated: points per LDS round of the streaming kernel for `total` bytes per point / per record"""
    t = total or 1
    c = (52 * 1024 // t) // 16 * 16
    if c < 1088 and 1088 * t <= 72 * 1024:
        c = 1088
    return min(c, 2048)


def filter_chunk(stride):
    """filter.hip's filter_chunk, restated: records per LDS chunk of the gather kernel"""
    return min(max((15 * 1024 // (stride or 1)) // 16 * 16, 16), 2048)


def test_round_sizes_restated():
    assert [stream_cap_for(b) for b in (1, 35, 41, 64, 96)] == [2048, 1520, 1296, 1088, 544]
    assert [filter_chunk(s) for s in (1, 41, 136, 20000)] == [2048, 368, 112, 16]


# ---- GPU: count and scan, called directly -------------------------------------------------------------------------------------------------------
def hostile_random(n, seed, density=0.5):
    rng = np.random.default_rng([seed, n])
    mask = np.asarray(HOSTILE, dtype=np.uint8)[rng.integers(0, len(HOSTILE), n)]
    mask[rng.random(n) >= density] = 0
    return mask


def count_and_scan(hooks, mask_dev, n):
    """launch_filter_count over the device bytes mask_dev[0, n) -> (counts, offsets with the total, the total_also word), as numpy arrays; the
    workspace has the size the product allocates, lies between guards and starts out filled with a pattern."""
    import torch
    tile = hooks.tile()
    assert tile == TILE
    n_tiles = -(-n // tile)
    size = hooks.workspace_bytes(n)
    assert size >= (n_tiles + 1) * 8 + n_tiles * 4
    block = torch.full((size + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = block.data_ptr() + GUARD
    offsets_at, counts_at = hooks.layout(ws, n, tile)
    assert offsets_at == ws and counts_at == ws + (n_tiles + 1) * 8
    also = torch.full((3,), -2, dtype=torch.int64, device="cuda")
    total_at = hooks.count(mask_dev.data_ptr(), n, tile, ws, torch.cuda.current_stream().cuda_stream, also.data_ptr() + 8)
    torch.cuda.synchronize()
    assert total_at == ws + n_tiles * 8
    host = block.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + size:] == FILL).all(), "the workspace's guards were written"
    offsets = host[GUARD:GUARD + (n_tiles + 1) * 8].view(np.uint64).copy()
    counts = host[GUARD + (n_tiles + 1) * 8:GUARD + (n_tiles + 1) * 8 + n_tiles * 4].view(np.uint32).copy()
    also = also.cpu().numpy()
    assert also[0] == -2 and also[2] == -2
    return counts, offsets, int(also[1])


def first_difference(got, expected):
    d = np.flatnonzero(got != expected)
    return f"{d.size} differ, first at {d[0]}: {got[d[0]]} != {expected[d[0]]}" if d.size else ""


def check_count_and_scan(hooks, mask_dev, mask_host):
    n = mask_host.size
    counts, offsets, also = count_and_scan(hooks, mask_dev, n)
    exp_counts = fr.tile_counts(mask_host)
    exp_offsets = fr.tile_offsets(exp_counts)
    assert counts.shape == exp_counts.shape and np.array_equal(counts, exp_counts), "counts: " + first_difference(counts, exp_counts)
    assert offsets.shape == exp_offsets.shape and np.array_equal(offsets, exp_offsets), "offsets: " + first_difference(offsets, exp_offsets)
    assert also == int(exp_offsets[-1])


def on_device(mask_host, offset=0):
    """the mask as device bytes at `offset` bytes from an aligned allocation, with selected-looking bytes all around it"""
    import torch
    n = mask_host.size
    big = torch.full((offset + n + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    view = big[offset:offset + n]
    view.copy_(torch.from_numpy(mask_host))
    assert view.data_ptr() % 16 == offset % 16
    return view


BYTE_N = 3 * 8192 + 777


def byte_value_mask(kind):
    if kind == "every":
        return (np.arange(BYTE_N) % 256).astype(np.uint8)
    if kind == "0x80":
        return np.full(BYTE_N, 0x80, dtype=np.uint8)
    if kind == "0xFF":
        return np.full(BYTE_N, 0xFF, dtype=np.uint8)
    assert kind == "one_byte_per_dword"  # a single non-zero byte in each dword position: the high bit alone, the low seven bits alone
    words = np.resize(np.array([0x00800000, 0x7F000000, 0x0000007F, 0x01000100], dtype="<u4"), -(-BYTE_N // 4))
    return words.view(np.uint8)[:BYTE_N].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["every", "0x80", "0xFF", "one_byte_per_dword"])
def test_count_every_byte_value(hip, hooks, kind):
    """mask[i] != 0 selects: three blocks of whole tiles on the four-tiles-per-wave path and 777 bytes on the vector loop and the byte tail."""
    mask = byte_value_mask(kind)
    check_count_and_scan(hooks, on_device(mask), mask)


SWITCH_N = [1, 15, 16, 17, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769] + [5 * 8192 + 2048 * k + 1 for k in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWITCH_N)
def test_count_fast_and_slow_path(hip, hooks, n):
    """A wave counts four whole tiles at once while (wave + 1) * 8192 <= n and walks its tiles one by one otherwise: n around every multiple of
    8192 up to one block of whole waves (32 768), and a block of fast waves, one more fast wave and a last wave of 0..3 whole tiles and one byte."""
    mask = hostile_random(n, 11)
    check_count_and_scan(hooks, on_device(mask), mask)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 3, 8, 13])
def test_count_unaligned_mask(hip, hooks, offset):
    mask = hostile_random(32769, 11)
    check_count_and_scan(hooks, on_device(mask, offset), mask)


SCAN_TILES = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 32767, 32768, 32769]
SCAN_CASES = [(t, tail, "random") for t in SCAN_TILES for tail in (0, 5)] + [(1025, 0, "full"), (4097, 0, "full"), (1025, 0, "empty"), (2049, 0, "last_byte")]


@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles,tail,kind", SCAN_CASES)
def test_scan_seams(hip, hooks, n_tiles, tail, kind):
    """The exclusive sum of the tile counts where the kernels change: up to 1024 tiles one block scans; beyond, every block of 1024 tiles sums the
    counts before its own (1025: a last block of one tile; 2047 / 2048 / 2049: a block border); the one-block scan (PST_FILTER_SCAN_BLOCKS=0,
    test_one_block_scan_at_the_same_sizes) takes rounds of 4096 tiles, eight of them loaded ahead (32 768).  Every tile full: a block's own counts
    sum to 1024 x 2048.  With a tail of 5 bytes the last tile is ragged and the tile count one more."""
    rng = np.random.default_rng([3, n_tiles, tail])
    if kind == "random":
        counts = rng.integers(0, TILE + 1, n_tiles)
    elif kind == "full":
        counts = np.full(n_tiles, TILE)
    else:
        counts = np.zeros(n_tiles, dtype=np.int64)
        if kind == "last_byte":
            counts[-1] = 1
    mask = fr.mask_with_counts(counts, tail, rng, HOSTILE, "last" if kind == "last_byte" else "run", tail_count=min(tail, 3))
    assert mask.size == n_tiles * TILE + tail and (kind != "last_byte" or (mask[-1] != 0 and np.count_nonzero(mask) == 1))
    check_count_and_scan(hooks, on_device(mask), mask)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles", [1 << 19, (1 << 19) + 1])
def test_scan_at_the_largest_many_block_size(hip, hooks, n_tiles):
    """2^19 tiles is the last size the many-block scan takes, 2^19 + 1 the first that goes back to one block (129 rounds).  Allocates a mask of
    1 GiB (+ 2 KiB) on the device, built there from the per-tile counts: mask[t * 2048 + j] = j < count[t] ? 0x80 : 0, and a workspace of 48 MiB."""
    import torch
    counts = np.random.default_rng([19, n_tiles]).integers(0, TILE + 1, n_tiles).astype(np.uint32)
    counts_dev = torch.from_numpy(counts.astype(np.int32)).cuda()
    mask = (torch.arange(TILE, dtype=torch.int32, device="cuda")[None, :] < counts_dev[:, None]).view(torch.uint8).mul_(0x80).reshape(-1)
    n = n_tiles * TILE
    assert mask.numel() == n and int(mask[:TILE].max().item()) in (0, 0x80)
    got_counts, got_offsets, also = count_and_scan(hooks, mask, n)
    del mask
    exp_offsets = fr.tile_offsets(counts)
    assert np.array_equal(got_counts, counts), "counts: " + first_difference(got_counts, counts)
    assert np.array_equal(got_offsets, exp_offsets), "offsets: " + first_difference(got_offsets, exp_offsets)
    assert also == int(exp_offsets[-1])


@pytest.mark.gpu
def test_one_block_scan_at_the_same_sizes():
    """PST_FILTER_SCAN_BLOCKS=0: every size of test_scan_seams through tile_scan_kernel (its rounds of 4096 tiles, its look-ahead of 32 768, the
    double-buffered wave totals).  The switch is read once per process, hence the child interpreter; it runs that one test function."""
    env = dict(os.environ, PST_FILTER_SCAN_BLOCKS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_filter_seams.py"), "-x", "-q", "-m", "gpu", "-k", "test_scan_seams",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    passed = re.search(r"(\d+) passed", r.stdout)
    assert passed and int(passed.group(1)) == len(SCAN_CASES) and "skipped" not in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]


# ---- GPU: the compaction end to end ------------------------------------------------------------------------------------------------------------
def packed(hip, types):
    return PointLayout.from_attributes_packed([PointAttributeDefinition(f"a{i}", t) for i, t in enumerate(types)], 1, api=hip)


def padded_narrow(hip):
    """the repr(C) layout of test_jit.py's test_specialised_compaction_keeps_the_padding_of_repr_c_records"""
    types = [("t", T.F32), ("i", T.U16), ("c", T.Vec3u8), ("k", T.U8), ("p", T.Vec3f32), ("b", T.ByteArray(5)), ("f", T.U8), ("g", T.U16), ("h", T.U8)]
    return PointLayout.from_attributes([PointAttributeDefinition(name, t) for name, t in types], api=hip)


def every_size(hip):
    """the 17 attributes of test_filter_append.py's test_filter_every_datatype_and_padding"""
    return PointLayout.from_attributes([PointAttributeDefinition(f"a{k}", T(k)) for k in range(16)] + [PointAttributeDefinition("blob", T.ByteArray(5))], api=hip)


def las0(hip):
    from pasture_amd import las
    return las.point_layout_from_las_point_format(las.Format(0), False, api=hip)


# name: (layout, bytes of the attributes or None, plan family, target kinds)
LAYOUTS = {
    "u8": (lambda hip: packed(hip, [T.U8]), 1, "jit", "HV"),
    "big": (custom_point_type_big, 41, "static", "HV"),
    "las0": (las0, 35, "static", "HV"),
    "bytes64": (lambda hip: packed(hip, [T.ByteArray(16)] * 4), 64, "jit", "HV"),
    "bytes96": (lambda hip: packed(hip, [T.ByteArray(16)] * 4 + [T.Vec3f64, T.U64]), 96, "jit", "V"),
    "padded": (padded_narrow, None, "jit", "V"),
    "every_size": (every_size, None, "interpreted", "HV"),
}
STATED_CAP = {"u8": 2048, "big": 1296, "las0": 1520, "bytes64": 1088, "bytes96": 544}
KINDS = {"H": HashMapBuffer, "V": VectorBuffer}


def round_size(name, layout, kind):
    """points per LDS round of the kernel this layout and target take"""
    attr_bytes = sum(a.size() for a in layout.attributes())
    stride = layout.size_of_point_entry()
    family = LAYOUTS[name][2]
    if family == "interpreted":
        return filter_chunk(stride)  # (the gather kernel has rounds for a record target only; the same counts serve its columnar form)
    cap = stream_cap_for(stride if kind == "V" else attr_bytes)
    if name in STATED_CAP:
        assert attr_bytes == stride == LAYOUTS[name][1] and cap == STATED_CAP[name], (name, attr_bytes, stride, cap)
    else:
        assert stride > attr_bytes  # (there IS padding)
    return cap


def seam_counts(cap):
    m = lambda c: min(c, TILE)
    return [cap - 1, cap, m(cap + 1), 0, TILE, 0, 1, 1, TILE - 1, m(2 * cap), m(2 * cap + 1), 16, 15, 17]


SEAM_POSITIONS = ["random"] * 6 + ["first", "last"] + ["random"] * 6
SEAM_TAIL = 777


def seam_mask(cap, tail_count, seed=0):
    counts = seam_counts(cap)
    mask = fr.mask_with_counts(counts, SEAM_TAIL, np.random.default_rng([5, cap, tail_count, seed]), HOSTILE, SEAM_POSITIONS, tail_count=tail_count)
    assert mask[6 * TILE] != 0 and mask[8 * TILE - 1] != 0 and fr.tile_counts(mask).tolist() == counts + [tail_count]
    return mask


def prefilled(kind, layout, count):
    dst = KINDS[kind].new_from_layout(layout)
    dst.resize(count)
    if count:
        raw = np.full((count, layout.size_of_point_entry()), UNWRITTEN, np.uint8)
        dst.set_point_range(range(0, count), raw.view(layout.numpy_record_dtype()).reshape(-1))
    return dst


def check_target(dst, kind, layout, expected, count, what=""):
    """dst's first len(expected) points are `expected`, bit for bit; everything else of its `count` points -- padding bytes of every record too --
    still holds what prefilled() put there"""
    k = len(expected)
    if kind == "H":
        for a in layout.attributes():
            col = np.ascontiguousarray(dst.get_attribute_range(a.attribute_definition(), range(0, count)))
            exp = np.ascontiguousarray(expected[a.name()])
            assert col[:k].nbytes == exp.nbytes, (what, a.name())
            width = max(1, col[:1].nbytes)
            bad = np.flatnonzero((col[:k].view(np.uint8).reshape(k, width) != exp.view(np.uint8).reshape(k, width)).any(axis=1))
            assert bad.size == 0, f"{what} {a.name()}: {bad.size} of {k} values differ, first at output point {bad[0]}"
            rest = col[k:].view(np.uint8)
            assert (rest == UNWRITTEN).all(), f"{what} {a.name()}: written beyond output point {k}"
        return
    got = np.ascontiguousarray(dst.get_point_range(range(0, count))).view(np.uint8).reshape(count, -1)
    covered = np.zeros(layout.size_of_point_entry(), bool)
    for a in layout.attributes():
        covered[a.offset():a.offset() + a.size()] = True
    exp = np.ascontiguousarray(expected).view(np.uint8).reshape(k, got.shape[1])
    bad = np.flatnonzero((got[:k][:, covered] != exp[:, covered]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {k} records differ, first at output point {bad[0]}"
    assert (got[:, ~covered] == UNWRITTEN).all(), f"{what}: padding bytes were written"
    assert (got[k:] == UNWRITTEN).all(), f"{what}: written beyond output point {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("tail_count", [0, SEAM_TAIL])
@pytest.mark.parametrize("name,kind", [(name, kind) for name, spec in LAYOUTS.items() for kind in spec[3]])
def test_compaction_at_the_round_seams(hip, jit_sync, name, kind, tail_count):
    """14 tiles holding cap - 1, cap, cap + 1, 0, 2048, 0, 1 (first byte), 1 (last byte), 2047, 2 cap, 2 cap + 1, 16, 15, 17 matches and a tail of
    777 points with none or all selected, cap being the points per LDS round of the kernel the layout takes (the chunk of the gather kernel): the
    rounds end exactly at, one before and one behind a tile's last match, and every tile from the second on starts at an odd output offset, so
    that neighbouring tiles share 16-byte spans of the target.  Device mask of hostile byte values; the target holds 0xAB before the call."""
    layout = LAYOUTS[name][0](hip)
    cap = round_size(name, layout, kind)
    mask = seam_mask(cap, tail_count)
    n = mask.size
    rec = random_records(layout, n, 31)
    src = HashMapBuffer.from_numpy(rec, layout)
    expected = fr.compact(rec, mask)
    k = len(expected)
    mask_dev = on_device(mask)
    dst = prefilled(kind, layout, k + 3)
    assert src.filter_into(dst, (mask_dev.data_ptr(), "device")) == k
    assert cv.last_plan_kinds(hip) == [LAYOUTS[name][2]], (name, kind, cv.last_plan_kinds(hip))
    check_target(dst, kind, layout, expected, k + 3, f"{name} into {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(name, kind) for name in ("big", "u8") for kind in "HV"])
def test_limit_at_the_seams(hip, jit_sync, name, kind):
    """filter_into_async with fewer points announced than the mask selects: exactly `hint` points are written -- the hint on a tile's first output
    point, one before and one behind it, on a round's end inside the full tile and one behind, 0, 1, total - 1, total -- and the count word
    says what the mask holds."""
    import torch
    layout = LAYOUTS[name][0](hip)
    cap = round_size(name, layout, kind)
    mask = seam_mask(cap, SEAM_TAIL)
    rec = random_records(layout, mask.size, 32)
    src = HashMapBuffer.from_numpy(rec, layout)
    offsets = [int(o) for o in fr.tile_offsets(fr.tile_counts(mask))]
    total = offsets[-1]
    assert seam_counts(cap)[4] == TILE  # (tile 4 is the full one: it has a round that ends at offsets[4] + cap)
    hints = [0, 1] + [offsets[t] + d for t in (1, 4, 5) for d in (-1, 0, 1)] + [offsets[4] + cap, offsets[4] + cap + 1, total - 1, total]
    assert all(0 <= h <= total for h in hints)
    mask_dev = on_device(mask)
    hits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    for hint in hints:
        dst = prefilled(kind, layout, total)
        hits.fill_(-1)
        src.filter_into_async(dst, mask_dev.data_ptr(), hint, hits.data_ptr())
        assert int(hits.item()) == total, hint
        if hint:
            assert cv.last_plan_kinds(hip) == [LAYOUTS[name][2]], (hint, cv.last_plan_kinds(hip))
        check_target(dst, kind, layout, fr.compact_limited(rec, mask, hint), total, f"{name} into {kind}, hint {hint}")


@pytest.mark.gpu
@pytest.mark.parametrize("selected", ["half", "all"])
@pytest.mark.parametrize("n", [1024 * TILE, 1025 * TILE + 5, 2049 * TILE + 5])
def test_whole_call_at_the_scan_seams(hip, jit_sync, n, selected):
    """One U8 column through filter(): the offsets of test_scan_seams as the scatter kernels use them -- 1024 tiles (one-block scan), 1025 and 2049
    tiles and a ragged one (many blocks), half of the points or all of them selected."""
    layout = LAYOUTS["u8"][0](hip)
    mask = hostile_random(n, 41, 0.5 if selected == "half" else 1.0)
    rec = random_records(layout, n, 42)
    src = HashMapBuffer.from_numpy(rec, layout)
    mask_dev = on_device(mask)
    out = src.filter(HashMapBuffer, (mask_dev.data_ptr(), "device"))
    assert cv.last_plan_kinds(hip) == ["jit"], cv.last_plan_kinds(hip)
    expected = fr.compact(rec, mask)
    assert out.len() == len(expected)
    check_target(out, "H", layout, expected, len(expected))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["H", "V"])
@pytest.mark.parametrize("offset", [1, 13])
def test_compaction_with_an_unaligned_device_mask(hip, kind, offset):
    """The scatter side reads the mask as dwords (streaming kernel) and qwords (gather kernel, the ragged tile): a mask at an odd address."""
    layout = custom_point_type_big(hip)
    n = 5 * TILE + 777
    mask = hostile_random(n, 51)
    rec = random_records(layout, n, 52)
    src = HashMapBuffer.from_numpy(rec, layout)
    expected = fr.compact(rec, mask)
    mask_dev = on_device(mask, offset)
    dst = prefilled(kind, layout, len(expected) + 3)
    assert src.filter_into(dst, (mask_dev.data_ptr(), "device")) == len(expected)
    assert cv.last_plan_kinds(hip) == ["static"], cv.last_plan_kinds(hip)
    check_target(dst, kind, layout, expected, len(expected) + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["H", "V"])
def test_host_mask_of_any_byte_values(hip, kind):
    """A host mask of dtype uint8 with values beyond 0 / 1 is copied to the device as it is: the same points as the device mask selects."""
    layout = custom_point_type_big(hip)
    n = 5 * TILE + 777
    mask = hostile_random(n, 61)
    assert mask.dtype == np.uint8 and mask.max() == 0xFF
    rec = random_records(layout, n, 62)
    src = HashMapBuffer.from_numpy(rec, layout)
    expected = fr.compact(rec, mask)
    from_host = src.filter(KINDS[kind], mask)
    mask_dev = on_device(mask)
    from_device = src.filter(KINDS[kind], (mask_dev.data_ptr(), "device"))
    assert from_host.len() == from_device.len() == len(expected)
    assert from_host.get_point_range(range(0, len(expected))).tobytes() == from_device.get_point_range(range(0, len(expected))).tobytes()
    check_target(from_host, kind, layout, expected, len(expected))
