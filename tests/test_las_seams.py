"""The LAS decoder (las_decode.hip), transposers (las_transpose.hip) and encoder (las_encode.hip) at their seams, bit for bit against the numpy
restatement of the LAS 1.4 record tables in las_ref.py -- a reference that shares nothing with pasture_amd/las.py or the oracle.

Inputs: uniformly random record BYTES (every field takes every bit pattern: NaN GPS times and waveform floats included) with planted rows of
extreme values; three scale / offset sets, one with negative scales, which together make -0.0 and +0.0 positions.  Sizes: every count around the
1024-point quad tile and around each multiple of 256 up to 2048 (the AoS / staged / strided tiles are multiples of 256), at range starts (0, 0) and
(1, 3); all sixteen source misalignments, each with another target misalignment, at n = 2051.  Every target is pre-filled with a sentinel and
compared WHOLE, so a byte written outside the target range fails like a wrong byte inside it.  Every device case asserts which kernel family ran
(last_plan_kinds) right after the call, before any read-back.  Floats are compared as bytes; there is no tolerance anywhere.  The conversions
run without and with the fused AABB (convert_into_with_bounds), whose bounds are compared bit for bit with the reference's sequential fold.

The two plans with two kernel families (raw records -> typed records, typed records -> columns) run twice: on the plan-specialised kernels in
process (run-time compiler in `sync` mode), and on the hand-written LAS kernels in ONE child process started with PST_LAS_PREFER_SPECIALISED=0 (the
switch is read once per process); the child is this module run as a script.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: the paths conftest.py sets up for the suite
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

import las_ref as R
from las_ref import (test_reference_decodes_the_fixtures_to_the_literal_vectors, test_reference_encode_of_decode_reproduces_the_fixture_bytes,  # noqa: F401
                     test_reference_equals_the_oracle_on_random_bytes)  # the reference's own pins run with the suite
from minmax_ref import assert_same_aabb, assert_same_bits, bounds_ref
from pasture_amd import conversion as cv
from pasture_amd import las
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.conversion import BufferLayoutConverter

F64_MAX = float(np.finfo(np.float64).max)
SEAMS = [1, 2, 3, 4, 5, 63, 64, 65] + [256 * j + d for j in range(1, 9) for d in (-1, 0, 1)] + [3 * 1024 + 7]
N_ALIGN = 2051
ALIGNMENTS = [(0, 0)] + [(i, (5 * i + 3) % 16) for i in range(16)]
# (n, first source point, first target point)
CASES = [(n, 0, 0) for n in SEAMS] + [(n, 1, 3) for n in SEAMS] + [(N_ALIGN, s0, t0) for s0, t0 in ALIGNMENTS]
N_SRC = 3088                      # >= max(s0 + n)
N_DST = max(t0 + n for n, _, t0 in CASES) + 5
SETS = [((0.001, 0.001, 0.001), (500000.0, 5400000.0, 100.0)),
        ((0.01, 0.25, 1.0 / 3.0), (0.0, -0.0, 1e-300)),
        ((-0.5, 0.125, -1e-3), (-0.0, 7.0, 0.0))]   # negative scales: X = 0 gives -0.0 * ... + -0.0 = -0.0, and -0.0 + 0.0 = +0.0
BLOCK = 256


def case_set(fmt, k):
    """Which scale / offset set case k of a format uses: all three meet every size over the formats."""
    return (k + fmt) % 3


# ---- the launchers' tile formulas, restated -------------------------------------------------------------------------------------------------
def tiles(fmt):
    rs, ts = R.RAW_SIZES[fmt], R.TYPED_SIZES[fmt]
    return {
        "decode quad": 4 * BLOCK,                                                 # las_decode.hip:26, :294 (kQuadTile)
        "decode aos": max(BLOCK, (48 * 1024 // (rs + ts)) // BLOCK * BLOCK),      # las_decode.hip:355-358 (las_decode_aos_tile)
        "transpose": 4 * BLOCK,                                                   # las_transpose.hip:21, :99, :201
        "encode quad": 4 * BLOCK,                                                 # las_encode.hip:452
        "encode staged": max(BLOCK, (48 * 1024 // (rs + ts)) // BLOCK * BLOCK),   # las_encode.hip:453
        "encode strided": max(BLOCK, (32 * 1024 // rs) // BLOCK * BLOCK),         # las_encode.hip:454
    }


@pytest.mark.parametrize("fmt", range(11))
def test_seams_bracket_every_tile(fmt):
    for name, t in tiles(fmt).items():
        assert t % BLOCK == 0 and {t - 1, t, t + 1} <= set(SEAMS), (fmt, name, t)
    aos = tiles(fmt)["decode aos"]
    assert 256 <= aos <= 768
    assert sorted({s0 * R.RAW_SIZES[fmt] % 16 for s0, _ in ALIGNMENTS}) == sorted({i * R.RAW_SIZES[fmt] % 16 for i in range(16)})
    assert sorted({t0 for _, t0 in ALIGNMENTS}) == list(range(16))  # every target start mod 16: every dmis a record size allows, every store phase


# ---- inputs (host side, computed once per format) -------------------------------------------------------------------------------------------
def planted_rows():
    """Absolute source rows that hold extreme values: 0, 3, 4, 255, 256, 1020-1027, the first and last point of each lane quad of wave 0 and
    wave 3 of the first tile, and the last four rows of every range -- for ranges that start at row 0 and at row 1."""
    base = {0, 3, 4, 255, 256} | set(range(1020, 1028))
    for wave in (0, 3):
        for lane in range(64 * wave, 64 * wave + 64):
            base |= {4 * lane, 4 * lane + 3}
    rows = set()
    for s0 in (0, 1):
        rows |= {p + s0 for p in base}
        for n in SEAMS + [N_ALIGN]:
            rows |= {s0 + n - k for k in range(1, 5) if s0 + n - k >= 0}
    return sorted(r for r in rows if r < N_SRC)


@functools.lru_cache(maxsize=None)
def raw_source(fmt):
    """(N_SRC, record size) uniformly random bytes with the planted rows."""
    rng = np.random.default_rng(90_000 + fmt)
    raw = rng.integers(0, 256, size=(N_SRC, R.RAW_SIZES[fmt]), dtype=np.uint8)
    rec = raw.view(R.RAW_DTYPES[fmt]).reshape(-1)
    rows = np.asarray(planted_rows())
    k = np.arange(rows.size)
    ext = np.array([R.INT32_MIN, -1, 0, 1, R.INT32_MAX], dtype=np.int32)
    rec["X"][rows], rec["Y"][rows], rec["Z"][rows] = ext[k % 5], ext[k // 5 % 5], ext[k // 25 % 5]
    u16 = np.where(k % 2 == 0, 0, 65535).astype(np.uint16)
    rec["intensity"][rows] = u16
    rec["point_source_id"][rows] = u16[::-1]
    if fmt <= 5:
        rec["flags"][rows] = k % 256
        rec["scan_angle_rank"][rows] = -128
    else:
        rec["flags0"][rows] = k % 256
        rec["flags1"][rows] = (7 * k + 3) % 256
        rec["scan_angle"][rows] = -32768
    for name in ("red", "green", "blue", "nir"):
        if name in rec.dtype.names:
            rec[name][rows] = u16
    assert rows.size >= 256
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def ref_columns(fmt, s):
    return R.decode(raw_source(fmt), fmt, *SETS[s])


@functools.lru_cache(maxsize=None)
def ref_typed(fmt, s):
    img = R.typed_records(ref_columns(fmt, s), fmt)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def typed_source(fmt):
    """Typed records of random BYTES for the transposers (pure byte moves): every field, positions included, takes every bit pattern."""
    img = np.random.default_rng(91_000 + fmt).integers(0, 256, size=(N_SRC, R.TYPED_SIZES[fmt]), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def sentinel(width):
    i = np.arange(N_DST * width, dtype=np.uint64)
    img = ((i * 37 + 11) % 251 + 1).astype(np.uint8).reshape(N_DST, width)  # never zero: a zero-filled target is not a sentinel
    img.setflags(write=False)
    return img


def test_both_zeros_occur_in_the_reference_positions():
    """The second and third scale / offset sets make -0.0 and +0.0 positions: without them the sign-of-zero rule of the bounds is idle."""
    for fmt in (0, 10):
        bits = np.concatenate([ref_columns(fmt, s)["Position3D"].view(np.uint64).reshape(-1) for s in (1, 2)])
        assert (bits == 0).any() and (bits == np.uint64(1) << np.uint64(63)).any()
        for s in (1, 2):  # and the planted extremes are there
            x = raw_source(fmt).view(R.RAW_DTYPES[fmt]).reshape(-1)["X"]
            assert {R.INT32_MIN, -1, 0, 1, R.INT32_MAX} <= set(x[planted_rows()].tolist())


# ---- the conversions ------------------------------------------------------------------------------------------------------------------------
OPS = {  # name: (source is raw records, source kind, target kind, kernel)
    "raw>H": (True, VectorBuffer, HashMapBuffer, "las_decode_kernel"),
    "raw>V": (True, VectorBuffer, VectorBuffer, "las_decode_aos_kernel"),
    "V>H": (False, VectorBuffer, HashMapBuffer, "las_records_to_columns_kernel"),
    "H>V": (False, HashMapBuffer, VectorBuffer, "las_columns_to_records_kernel"),
}


def layouts(api, fmt):
    raw = las.point_layout_from_las_point_format(las.Format(fmt), True, api=api)
    typed = las.point_layout_from_las_point_format(las.Format(fmt), False, api=api)
    assert raw.size_of_point_entry() == R.RAW_SIZES[fmt]
    R.check_typed_layout(typed, fmt)
    return raw, typed


def run_conversions(api, fmt, op, with_bounds=False, cases=None):
    """Runs every case of (format, op) and yields (k, whole target image, plan kinds or None, bounds or None).  One source buffer and one target
    buffer per call; the target is re-filled with the sentinel before every case."""
    from_raw, src_kind, dst_kind, _ = OPS[op]
    raw_l, typed_l = layouts(api, fmt)
    ts = R.TYPED_SIZES[fmt]
    src = src_kind.from_numpy(raw_source(fmt) if from_raw else typed_source(fmt), raw_l if from_raw else typed_l)
    dst = dst_kind.new_from_layout(typed_l)
    dst.resize(N_DST)
    convs = {}
    for k, (n, s0, t0) in enumerate(CASES if cases is None else cases):
        s = case_set(fmt, k)
        if s not in convs:
            convs[s] = las.get_default_las_converter(raw_l, typed_l, *SETS[s]) if from_raw else BufferLayoutConverter.for_layouts(typed_l, typed_l)
        dst.set_point_range(range(0, N_DST), sentinel(ts))
        bounds = None
        if with_bounds:
            bounds = convs[s].convert_into_with_bounds(src, dst, range(s0, s0 + n), range(t0, t0 + n))
        else:
            convs[s].convert_into_range(src, range(s0, s0 + n), dst, range(t0, t0 + n))
        kinds = cv.last_plan_kinds(api) if api.is_product else None  # before the read-back: reading columns as records is a conversion too
        yield k, whole_image(dst, typed_l, fmt), kinds, bounds


def whole_image(buf, typed_l, fmt):
    """Every byte of a typed buffer as (points, typed size): records as they lie; columns read ONE BY ONE (a plain copy of each column, no
    kernel of the kind under test in between) and laid side by side on the host."""
    if buf.as_columnar() is None:
        return buf.get_point_range(range(0, buf.len()))
    return R.typed_records({a.name(): buf.view_attribute(a.attribute_definition()) for a in typed_l.attributes()}, fmt)


def expected_image(fmt, op, k, case):
    n, s0, t0 = case
    want = sentinel(R.TYPED_SIZES[fmt]).copy()
    rows = ref_typed(fmt, case_set(fmt, k)) if OPS[op][0] else typed_source(fmt)
    want[t0:t0 + n] = rows[s0:s0 + n]
    return want


def assert_image(got, want, fmt, what, typed=True):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    row, byte = (int(v) for v in np.argwhere(got != want)[0])
    raise AssertionError(f"format {fmt} {what}: {int((got != want).any(axis=1).sum())} rows differ; first: target row {row} byte {byte} "
                         f"({R.field_at(fmt, byte, typed)}): got {got[row].tobytes().hex()} want {want[row].tobytes().hex()}")


def check_conversions(api, fmt, op, with_bounds=False, expect_kinds=None, seen=None):
    for k, img, kinds, bounds in run_conversions(api, fmt, op, with_bounds):
        case = CASES[k]
        what = f"{op} ({OPS[op][3]}) case {k} (n, s0, t0) = {case} set {case_set(fmt, k)} kinds {kinds}"
        if api.is_product:
            assert kinds and "none" not in kinds, what
            if expect_kinds is not None:
                assert kinds == expect_kinds, what
            if seen is not None:
                seen.setdefault(tuple(kinds), []).append(case)
        assert_image(img, expected_image(fmt, op, k, case), fmt, what)
        if with_bounds:
            n, s0, _ = case
            assert bounds is not None, what
            assert_same_aabb(bounds, expected_bounds(fmt, op, k, case), what)


@functools.lru_cache(maxsize=None)
def typed_source_positions(fmt):
    return R.typed_columns(typed_source(fmt), fmt)["Position3D"]


def expected_bounds(fmt, op, k, case):
    """calculate_bounds of the target range, restated (minmax_ref.bounds_ref).  The transposers' random bytes make NaN, infinite and subnormal
    positions: a NaN never wins a strict compare, so it is never a bound."""
    n, s0, _ = case
    pos = ref_columns(fmt, case_set(fmt, k))["Position3D"] if OPS[op][0] else typed_source_positions(fmt)
    return bounds_ref(pos[s0:s0 + n])


@pytest.mark.parametrize("fmt", range(11))
def test_raw_records_to_columns(api, fmt):
    """las_decode_kernel: one family."""
    check_conversions(api, fmt, "raw>H", expect_kinds=["las-specialised"])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", range(11))
def test_raw_records_to_columns_with_bounds(hip, fmt):
    """las_decode_kernel with the fused AABB: the bounds of the target range bit for bit, the sign of a zero bound included."""
    check_conversions(hip, fmt, "raw>H", with_bounds=True, expect_kinds=["las-specialised"])


@pytest.mark.parametrize("fmt", range(11))
def test_columns_to_typed_records(api, fmt):
    """las_columns_to_records_kernel: the default for columns -> typed records."""
    check_conversions(api, fmt, "H>V", expect_kinds=["las-specialised"])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", range(11))
def test_columns_to_typed_records_with_bounds(hip, fmt):
    """las_columns_to_records_kernel with the fused AABB of the positions it moves."""
    check_conversions(hip, fmt, "H>V", with_bounds=True, expect_kinds=["las-specialised"])


@pytest.mark.parametrize("op", ["raw>V", "V>H"])
@pytest.mark.parametrize("fmt", range(11))
def test_two_family_plans_on_the_oracle(oracle, fmt, op):
    """The CPU leg of the two plans below: pins the oracle (and pasture_amd/las.py) against the numpy reference at the same cases."""
    check_conversions(oracle, fmt, op)


@pytest.fixture
def jit_sync(hip):
    cv.jit_set_mode("sync", api=hip)
    yield
    cv.jit_set_mode("env", api=hip)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bounds", [False, True])
@pytest.mark.parametrize("op", ["raw>V", "V>H"])
@pytest.mark.parametrize("fmt", range(11))
def test_two_family_plans_on_the_plan_specialised_kernels(hip, jit_sync, fmt, op, with_bounds):
    """Raw records -> typed records and typed records -> columns with the plan-specialised kernel compiled inside the call (`sync`): aligned
    whole tiles take `jit` or `static`; misaligned ranges and the ragged tail take whatever serves them -- never nothing."""
    seen = {}
    check_conversions(hip, fmt, op, with_bounds=with_bounds, seen=seen)
    print(f"format {fmt} {op} bounds {with_bounds}: " + "; ".join(f"{'+'.join(k)}: {len(cs)} cases, (s0, t0) in {sorted({c[1:] for c in cs})}" for k, cs in seen.items()))
    assert seen and all(k and "none" not in k for k in seen), seen
    aligned = [k for k, cs in seen.items() if (SEAMS[-1], 0, 0) in cs]
    assert len(aligned) == 1 and ({"jit", "static"} & set(aligned[0])), (fmt, op, seen)


@pytest.fixture(scope="module")
def las_family_child(tmp_path_factory):
    """The whole matrix of the two plans on the hand-written LAS kernels, in one fresh process with PST_LAS_PREFER_SPECIALISED=0."""
    out = tmp_path_factory.mktemp("las_family") / "results.npz"
    env = dict(os.environ, PST_LAS_PREFER_SPECIALISED="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    data = np.load(out)
    yield data
    data.close()
    os.remove(out)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["raw>V", "V>H"])
@pytest.mark.parametrize("fmt", range(11))
def test_two_family_plans_on_the_las_kernels(las_family_child, fmt, op):
    """las_decode_aos_kernel and las_records_to_columns_kernel themselves, without and with the fused AABB: every call of the child reported
    the LAS family."""
    flat, kinds, rest = (las_family_child[f"{fmt}_{op}{suffix}"] for suffix in ("", "_kinds", "_rest"))
    ts = R.TYPED_SIZES[fmt]
    assert len(kinds) == len(CASES) == len(rest) and flat.size == sum(kept_rows(c) for c in CASES) * ts
    at = 0
    for k, case in enumerate(CASES):
        what = f"{op} ({OPS[op][3]}) LAS family, case {k} (n, s0, t0) = {case} kinds {kinds[k]}"
        assert str(kinds[k]) == "las-specialised", what
        rows = kept_rows(case)
        assert_image(flat[at:at + rows * ts].reshape(rows, ts), expected_image(fmt, op, k, case)[:rows], fmt, what)
        assert rest[k], what + ": bytes beyond the kept rows changed"
        at += rows * ts
    bmin, bmax, bkinds, bsame = (las_family_child[f"{fmt}_{op}{suffix}"] for suffix in ("_bmin", "_bmax", "_bkinds", "_bsame"))
    assert len(bmin) == len(bmax) == len(bkinds) == len(bsame) == len(CASES)
    for k, case in enumerate(CASES):
        what = f"{op} ({OPS[op][3]}) LAS family with bounds, case {k} (n, s0, t0) = {case} kinds {bkinds[k]}"
        assert str(bkinds[k]) == "las-specialised", what
        assert bsame[k], what + ": the target differs from the one the call without bounds left (which is compared above)"
        assert_same_aabb((bmin[k].view(np.float64), bmax[k].view(np.float64)), expected_bounds(fmt, op, k, case), what)


def kept_rows(case):
    """Rows of the target image the child hands over whole: the range, everything before it and five rows after it.  (The rows beyond are
    sentinel rows; the child says whether they still are -- all of them would be 300 MB.)"""
    n, _, t0 = case
    return t0 + n + 5


def child_main(out_path):
    from pasture_amd import product_api
    api = product_api()
    assert os.environ.get("PST_LAS_PREFER_SPECIALISED") == "0"
    results = {}
    for fmt in range(11):
        for op in ("raw>V", "V>H"):
            imgs, kinds, rest, whole = [], [], [], []
            for k, img, kd, _ in run_conversions(api, fmt, op):
                whole.append(img)
                rows = kept_rows(CASES[k])
                imgs.append(img[:rows].reshape(-1))
                rest.append(bool(np.array_equal(img[rows:], sentinel(R.TYPED_SIZES[fmt])[rows:])))
                kinds.append(",".join(kd))
            results[f"{fmt}_{op}"] = np.concatenate(imgs)
            results[f"{fmt}_{op}_kinds"] = np.asarray(kinds)
            results[f"{fmt}_{op}_rest"] = np.asarray(rest)
            # the same cases with the fused AABB: bounds as bits, and whether the target came out as it did without
            bmin, bmax, bkinds, bsame = [], [], [], []
            for k, img, kd, b in run_conversions(api, fmt, op, with_bounds=True):
                bmin.append(np.asarray(b.min(), dtype=np.float64).view(np.uint64))
                bmax.append(np.asarray(b.max(), dtype=np.float64).view(np.uint64))
                bkinds.append(",".join(kd))
                bsame.append(bool(np.array_equal(img, whole[k])))
            results[f"{fmt}_{op}_bmin"], results[f"{fmt}_{op}_bmax"] = np.stack(bmin), np.stack(bmax)
            results[f"{fmt}_{op}_bkinds"], results[f"{fmt}_{op}_bsame"] = np.asarray(bkinds), np.asarray(bsame)
    np.savez(out_path, **results)


# ---- n = 0 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(OPS))
def test_empty_range_leaves_the_target_untouched(api, op):
    fmt = 3
    for k, img, kinds, bounds in run_conversions(api, fmt, op, with_bounds=api.is_product, cases=[(0, 0, 0), (0, 5, 7)]):
        assert_image(img, sentinel(R.TYPED_SIZES[fmt]), fmt, f"{op} empty range {k}")
        assert bounds is None
        if api.is_product:
            assert set(kinds) <= {"none"}, kinds  # nothing was launched, and the call says so


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder_columns(fmt, s, draw):
    """Source columns of the encoder.  draw 0: decode of the random raw bytes -- on the LAS grid and in range by construction.  draw 1: positions
    OFF the grid, uniform over the in-range interval of locals (negative ones included: truncation toward zero), the largest and the smallest
    in-range local planted, and the bit-field columns with all eight bits random (the encoder keeps the low ones).
    In range means: trunc((p - offset) / scale) as i64 lies in [i32::MIN, i32::MAX] -- oracle/oracle_capi.cpp:559-563, the restatement of
    write_position_as_las_position (write_helpers.rs:10-23)."""
    cols = dict(ref_columns(fmt, s))
    if draw == 1:
        rng = np.random.default_rng(92_000 + 16 * fmt + s)
        sc, of = np.asarray(SETS[s][0]), np.asarray(SETS[s][1])
        local = rng.uniform(-2147483648.9, 2147483647.9, size=(N_SRC, 3))
        local[::7] = rng.uniform(-3.0, 3.0, size=local[::7].shape)
        p = local * sc + of
        extremes = np.array([2147483647.5, -2147483648.5])
        for row in (5, 1029, 2050):
            p[row] = extremes[0] * sc + of
            p[row + 1] = extremes[1] * sc + of
        with np.errstate(over="ignore", invalid="ignore"):
            t = np.trunc((p - of) / sc)
        ok = np.isfinite(t) & (t >= R.INT32_MIN) & (t <= R.INT32_MAX)
        p = np.where(ok, p, np.broadcast_to(of, p.shape))
        cols["Position3D"] = np.ascontiguousarray(p)
        for name in ("ReturnNumber", "NumberOfReturns", "ClassificationFlags", "ScannerChannel", "ScanDirectionFlag", "EdgeOfFlightLine"):
            if name in cols:
                cols[name] = rng.integers(0, 256, size=N_SRC, dtype=np.uint8)
    return cols


@functools.lru_cache(maxsize=None)
def encoder_records(fmt, s, draw):
    img = R.encode(encoder_columns(fmt, s, draw), fmt, *SETS[s])
    img.setflags(write=False)
    return img


def test_encoder_inputs_reach_the_edges():
    for s in range(3):
        x = encoder_records(0, s, 1).view(R.RAW_DTYPES[0]).reshape(-1)
        for a in "XYZ":
            assert x[a].max() == R.INT32_MAX and x[a].min() == R.INT32_MIN and (x[a] == 0).any() and (x[a] < 0).any(), (s, a)
        local = (encoder_columns(0, s, 1)["Position3D"] - np.asarray(SETS[s][1])) / np.asarray(SETS[s][0])
        assert ((local < 0) & (local > -3) & (local != np.trunc(local))).any()  # where truncation and flooring differ


HEADER_SEEDS = [F64_MAX, 0.0, -0.0, -0.0, -F64_MAX, 0.0]  # identities, and zeros of both signs that come first among equal bounds


def check_encoder(api, fmt, src_kind):
    raw_l, typed_l = layouts(api, fmt)
    rs = R.RAW_SIZES[fmt]
    srcs = {}
    dst = VectorBuffer.new_from_layout(raw_l)
    dst.resize(N_DST)
    for k, (n, s0, t0) in enumerate(CASES):
        s = case_set(fmt, k)
        for draw in (0, 1):
            if (s, draw) not in srcs:
                srcs[(s, draw)] = src_kind.from_numpy(R.typed_records(encoder_columns(fmt, s, draw), fmt), typed_l)
            seeds = HEADER_SEEDS if (k + draw) % 2 else None
            max_return = 5 if (k // 2 + draw) % 2 else 15
            dst.set_point_range(range(0, N_DST), sentinel(rs))
            bounds, counts = las.encode_points(srcs[(s, draw)].slice(range(s0, s0 + n)), fmt, *SETS[s], dst, target_first=t0, header_bounds=seeds,
                                               max_return=max_return)
            what = f"encoder from {src_kind.__name__} case {k} (n, s0, t0) = {(n, s0, t0)} set {s} draw {draw} seeds {seeds is not None} max_return {max_return}"
            want = sentinel(rs).copy()
            want[t0:t0 + n] = encoder_records(fmt, s, draw)[s0:s0 + n]
            assert_image(dst.get_point_range(range(0, N_DST)), want, fmt, what, typed=False)
            cols = R.slice_columns(encoder_columns(fmt, s, draw), s0, s0 + n)
            wmin, wmax = R.header_bounds(cols, seeds)
            assert_same_bits(np.asarray(bounds[0]), wmin, what + " (min)")
            assert_same_bits(np.asarray(bounds[1]), wmax, what + " (max)")
            assert counts == R.return_counts(cols, max_return), what


@pytest.mark.parametrize("src_kind", [HashMapBuffer, VectorBuffer])
def test_encoder_of_no_points_leaves_target_and_header_as_they_were(api, src_kind):
    fmt = 8
    raw_l, typed_l = layouts(api, fmt)
    src = src_kind.from_numpy(R.typed_records(encoder_columns(fmt, 0, 0), fmt), typed_l)
    dst = VectorBuffer.from_numpy(sentinel(R.RAW_SIZES[fmt]), raw_l)
    for seeds in (None, HEADER_SEEDS):
        bounds, counts = las.encode_points(src.slice(range(9, 9)), fmt, *SETS[0], dst, target_first=7, header_bounds=seeds)
        assert_image(dst.get_point_range(range(0, N_DST)), sentinel(R.RAW_SIZES[fmt]), fmt, "empty encode", typed=False)
        wmin, wmax = R.header_bounds(R.slice_columns(encoder_columns(fmt, 0, 0), 9, 9), seeds)
        assert_same_bits(np.asarray(bounds[0]), wmin, "min")
        assert_same_bits(np.asarray(bounds[1]), wmax, "max")
        assert counts == [0] * 15


@pytest.mark.parametrize("fmt", range(11))
def test_encoder_from_columns(api, fmt):
    """las_encode_kernel<MODE_QUAD>: full tiles take encode_quad_tile, the ragged tile the per-point path.  (MODE_STRIDED has no public route:
    a columnar buffer's stride is always the element size and an interleaved one is staged, las_api.cpp / runtime.hpp attr_view.)"""
    check_encoder(api, fmt, HashMapBuffer)


@pytest.mark.parametrize("fmt", range(11))
def test_encoder_from_records(api, fmt):
    """las_encode_kernel<MODE_STAGED>: typed records staged in LDS at any alignment."""
    check_encoder(api, fmt, VectorBuffer)


# ---- the fold seams (format 0) --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_decoder_bounds_fold_goes_two_level(hip):
    """More than 4096 block records: launch_finalize_bounds folds in two levels (stream.hip).  Raw -> columns has one family, so nothing is measured."""
    fmt, s = 0, 1
    n = 4096 * 1024 + 1025
    raw = np.random.default_rng(93_000).integers(0, 256, size=(n, R.RAW_SIZES[fmt]), dtype=np.uint8)
    rec = raw.view(R.RAW_DTYPES[fmt]).reshape(-1)
    rec["X"][[7, n - 3]] = 0          # zeros of either sign are possible bounds only if nothing lies beyond them; they are folded all the same
    rec["Y"][n - 1], rec["Z"][n - 1025] = R.INT32_MAX, R.INT32_MIN  # extremes in the last (ragged) tile and in the last full one
    raw_l, typed_l = layouts(hip, fmt)
    src = VectorBuffer.from_numpy(raw, raw_l)
    dst = HashMapBuffer.new_from_layout(typed_l)
    dst.resize(n)
    b = las.get_default_las_converter(raw_l, typed_l, *SETS[s]).convert_into_with_bounds(src, dst)
    assert cv.last_plan_kinds(hip) == ["las-specialised"]
    want = R.decode(raw, fmt, *SETS[s])
    assert_same_aabb(b, bounds_ref(want["Position3D"]), "two-level fold")
    for a in typed_l.attributes():
        assert dst.view_attribute(a.attribute_definition()).tobytes() == want[a.name()].tobytes(), a.name()


@pytest.mark.gpu
@pytest.mark.parametrize("src_kind", ["H", "V"])
def test_encoder_fold_goes_two_level(hip, src_kind):
    """More than 256 tiles: the encoder's fold goes two-level (las_encode.hip:483).  From columns the tile is 1024 points, from format-0 records 768."""
    fmt, s = 0, 0
    tile = tiles(fmt)["encode quad" if src_kind == "H" else "encode staged"]
    n = 256 * tile + tile + 1
    raw = np.random.default_rng(94_000).integers(0, 256, size=(n, R.RAW_SIZES[fmt]), dtype=np.uint8)
    cols = R.decode(raw, fmt, *SETS[s])
    raw_l, typed_l = layouts(hip, fmt)
    src = (HashMapBuffer if src_kind == "H" else VectorBuffer).from_numpy(R.typed_records(cols, fmt), typed_l)
    dst = VectorBuffer.new_from_layout(raw_l)
    dst.resize(n)
    bounds, counts = las.encode_points(src, fmt, *SETS[s], dst, max_return=5)
    assert dst.get_point_range(range(0, n)).tobytes() == R.encode(cols, fmt, *SETS[s]).tobytes()
    wmin, wmax = R.header_bounds(cols)
    assert_same_bits(np.asarray(bounds[0]), wmin, "min")
    assert_same_bits(np.asarray(bounds[1]), wmax, "max")
    assert counts == R.return_counts(cols, 5)


if __name__ == "__main__":
    child_main(sys.argv[1])
