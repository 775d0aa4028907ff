"""Gather by index and the device sort orders (pst_buffer_gather / _async / pst_buffer_take, pst_sort_order_by_attribute_device,
pst_morton_order_device, pst_shuffle_order_device, pst_invert_order_device) against tests/reorder_ref.py.

CPU tests pin the restatement (the keys against np.argsort, the Morton order against a Z-order written by hand) and the argument checks that
are answered on the host.  GPU tests compare bytes and orders with np.array_equal: a gather moves bytes and a sort order is a function of
the keys alone, so there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import reorder_ref as R
from pasture_amd import PastureError, PasturePanic
from pasture_amd import algorithms as alg
from pasture_amd.buffers import ExternalMemoryBuffer, HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition as Def, PointLayout, attributes as A

PPB = 256           # points_per_block, asserted against pst_reorder_kernel_shape below: the parametrisations need it at collection time
TILE_BYTES = 32768  # record_tile_bytes
LENGTHS = [0, 1, 2, 63, 64, 65, PPB - 1, PPB, PPB + 1, 3 * PPB + 17]
BIG = 200_003       # the multi-pass sorts
KINDS = {"V": VectorBuffer, "H": HashMapBuffer}
SCALARS = {"U8": T.U8, "I8": T.I8, "U16": T.U16, "I16": T.I16, "U32": T.U32, "I32": T.I32, "U64": T.U64, "I64": T.I64, "F32": T.F32, "F64": T.F64}


# ------------------------------------------------------------------------------------------------------------------------------- layouts

def layout_of(name, hip):
    blob5, blob12k = Def.custom("Blob", T.ByteArray(5)), Def.custom("Blob", T.ByteArray(12000))
    las_like = [A.POSITION_3D, A.INTENSITY, A.RETURN_NUMBER, A.NUMBER_OF_RETURNS, A.CLASSIFICATION, A.SCAN_ANGLE_RANK, A.USER_DATA,
                A.POINT_SOURCE_ID, A.GPS_TIME, A.WAVEFORM_PACKET_SIZE]  # ten attributes of 24, 2, 1, 1, 1, 1, 1, 2, 8 and 4 bytes
    if name == "xyz":
        return PointLayout.from_attributes([A.POSITION_3D], api=hip)
    if name == "las":
        return PointLayout.from_attributes(las_like, api=hip)
    if name == "las_packed":  # the Vec3f64 at byte offset 1
        return PointLayout.from_attributes_packed([A.CLASSIFICATION] + [a for a in las_like if a is not A.CLASSIFICATION], 1, api=hip)
    if name == "blob5":
        return PointLayout.from_attributes([A.POSITION_3D, blob5, A.INTENSITY], api=hip)
    if name == "blob12k":
        return PointLayout.from_attributes_packed([A.INTENSITY, blob12k, A.POSITION_3D], 1, api=hip)
    raise KeyError(name)


def records(layout, n, seed):
    """n records of random bytes: every attribute byte and every padding byte"""
    return np.random.default_rng(seed).integers(0, 256, (n, layout.size_of_point_entry()), dtype=np.uint8)


def filled(kind, layout, rec):
    buf = KINDS[kind].new_from_layout(layout)
    if len(rec):
        buf.resize(len(rec))
        buf.set_point_range(range(0, len(rec)), rec)
    return buf


def all_records(buf):
    return buf.get_point_range(range(0, buf.len()))


def written_bytes(layout, src_kind, dst_kind):
    """the bytes of a target record a gather of this pairing writes: whole records between two interleaved buffers, else the attributes"""
    return None if (src_kind, dst_kind) == ("V", "V") else R.attribute_byte_mask(layout)


def index_patterns(n, rng):
    """(name, indices) for a source of n points"""
    if n == 0:
        return [("empty", np.zeros(0, dtype=np.int64))]
    return [("identity", np.arange(n)), ("reverse", np.arange(n)[::-1].copy()), ("permutation", rng.permutation(n)),
            ("broadcast", np.full(n, n // 2)), ("repeats_long", rng.integers(0, n, 2 * n + 3)), ("repeats_short", rng.integers(0, n, n // 3))]


class DeviceIndices:
    """an index list in device memory, as the (device_ptr, count, bits) triple the buffers take"""

    def __init__(self, idx, bits):
        import torch
        arr = np.ascontiguousarray(idx).astype(np.uint32 if bits == 32 else np.uint64)
        self.t = torch.from_numpy(arr.view(np.int32 if bits == 32 else np.int64).copy()).cuda()
        self.triple = (self.t.data_ptr() if arr.size else 0, arr.size, bits)


def index_forms(idx, case):
    """the list as (what the buffers take, keepalive): both widths, host and device memory, i64 as numpy hands it out -- by turns"""
    form = case % 5
    if form == 0:
        return np.asarray(idx, dtype=np.int64), None
    if form == 1:
        return np.asarray(idx).astype(np.uint32), None
    if form == 2:
        return np.asarray(idx).astype(np.uint64), None
    d = DeviceIndices(idx, 32 if form == 3 else 64)
    return d.triple, d


# ------------------------------------------------------------------------------------------------------------------- the restatement (CPU)

def special_values(dtype, n, seed):
    """n values of a numeric dtype with heavy ties, the extremes, and for floats signed zeros, infinities and NaNs of both signs"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        v = rng.normal(0, 100, n).astype(dtype)
        ties = rng.random(n) < 0.3
        v[ties] = rng.integers(-3, 4, int(ties.sum())).astype(dtype)
        specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, np.finfo(dtype).max, np.finfo(dtype).min, np.finfo(dtype).tiny, -np.finfo(dtype).tiny],
                            dtype=dtype)
        specials[5] = np.copysign(specials[4], -1)  # a NaN with the sign bit set
        at = rng.random(n) < 0.2
        v[at] = specials[rng.integers(0, len(specials), int(at.sum()))]
        return v
    info = np.iinfo(dtype)
    v = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    ties = rng.random(n) < 0.5
    v[ties] = rng.integers(max(info.min, -3), 4, int(ties.sum())).astype(dtype)
    at = rng.random(n) < 0.1
    v[at] = np.array([info.min, info.max, 0], dtype=dtype)[rng.integers(0, 3, int(at.sum()))]
    return v


@pytest.mark.parametrize("name", list(SCALARS))
def test_keys_reproduce_numpy_stable_argsort(name):
    dtype = SCALARS[name].numpy_dtype()
    for n, seed in ((0, 1), (1, 2), (1000, 3), (5000, 4)):
        v = special_values(dtype, n, seed)
        if dtype.kind == "f" and n >= 1000:
            assert np.isnan(v).any() and np.signbit(v[np.isnan(v)]).any() and not np.signbit(v[np.isnan(v)]).all()
            assert (v == 0).any() and np.signbit(v[v == 0]).any() and np.isinf(v).any()
        keys = R.attribute_keys(v)
        assert keys.dtype == np.dtype(f"<u{dtype.itemsize}")
        assert np.array_equal(R.argsort_attribute(v), np.argsort(v, kind="stable")), (name, n)


@pytest.mark.parametrize("name", list(SCALARS))
def test_descending_keeps_ties_in_input_order_and_nans_last(name):
    dtype = SCALARS[name].numpy_dtype()
    v = special_values(dtype, 3000, 7)
    order = R.argsort_attribute(v, descending=True).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(len(v)))
    s = v[order]
    nan = np.isnan(s) if dtype.kind == "f" else np.zeros(len(s), dtype=bool)
    m = int((~nan).sum())
    assert not nan[:m].any() and nan[m:].all(), "NaNs last"
    assert np.array_equal(order[m:], np.flatnonzero(np.isnan(v) if dtype.kind == "f" else nan)), "NaNs in input order"
    assert (s[:m - 1] >= s[1:m]).all(), "descending"
    same = s[:m - 1] == s[1:m]  # (-0.0 == +0.0: a tie)
    assert (order[:m - 1][same] < order[1:m][same]).all(), "ties in input order"


def test_morton_reference_on_a_lattice_is_the_z_order_written_by_hand():
    """4 x 4 x 4 lattice, two bits per axis: the Z-order is the nested quads -- the high bits of z, y, x, then the low bits, x fastest"""
    z_order = [(2 * x1 + x0, 2 * y1 + y0, 2 * z1 + z0) for z1 in (0, 1) for y1 in (0, 1) for x1 in (0, 1) for z0 in (0, 1) for y0 in (0, 1) for x0 in (0, 1)]
    assert z_order[:9] == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (2, 0, 0)] and z_order[-1] == (3, 3, 3)
    rng = np.random.default_rng(5)
    P = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], dtype=np.float64)[rng.permutation(64)]
    P = P * np.array([0.5, 3.0, 100.0]) + np.array([-7.0, 1e6, 0.25])  # the key does not depend on the box
    order = R.morton_order(P, 3, 2)
    back = np.rint((P[order] - np.array([-7.0, 1e6, 0.25])) / np.array([0.5, 3.0, 100.0])).astype(int)
    assert [tuple(p) for p in back] == z_order
    assert np.array_equal(R.morton_keys(P, 3, 2)[order], np.arange(64, dtype=np.uint64))
    # two axes: x and y only, z ignored; ties (the four z of a column) in input order
    order2 = R.morton_order(P, 2, 2)
    quads = [(2 * x1 + x0, 2 * y1 + y0) for y1 in (0, 1) for x1 in (0, 1) for y0 in (0, 1) for x0 in (0, 1)]
    back2 = np.rint((P[order2] - np.array([-7.0, 1e6, 0.25])) / np.array([0.5, 3.0, 100.0])).astype(int)
    assert [tuple(p[:2]) for p in back2[::4]] == quads
    for g in range(16):
        assert (np.diff(order2[4 * g:4 * g + 4].astype(int)) > 0).all()
    # the clamps: the max face is the last cell; points that are not finite have the key 1 << 63 and come last in input order
    Q = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [0.5, 0.5, 0.5], [0, np.inf, 0], [1, 0, 0]], dtype=np.float64)
    k = R.morton_keys(Q, 3, 3)
    assert k.tolist() == [0, 0b111111111, 1 << 63, 0b111000000, 1 << 63, 0b001001001]
    assert R.morton_order(Q, 3, 3).tolist() == [0, 5, 3, 1, 2, 4]
    assert R.morton_keys(np.full((3, 3), np.nan)).tolist() == [1 << 63] * 3 and R.morton_keys(np.zeros((0, 3))).shape == (0,)
    assert R.morton_keys(np.ones((4, 3))).tolist() == [0] * 4  # one point repeated: inv = 0


def test_reference_shuffle_and_gather():
    assert int(R.splitmix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF  # the published first output of splitmix64 from state 0
    order = R.shuffle_order(1000, 9)
    assert np.array_equal(np.sort(order), np.arange(1000)) and not np.array_equal(order, np.arange(1000))
    assert np.array_equal(R.invert(order)[order], np.arange(1000))
    src = np.arange(40, dtype=np.uint8).reshape(10, 4)
    dst = np.full((6, 4), 255, dtype=np.uint8)
    out = R.gather(src, [9, 0, 9], dst, 2, byte_mask=np.array([True, False, True, True]))
    assert out.tolist() == [[255] * 4, [255] * 4, [36, 255, 38, 39], [0, 255, 2, 3], [36, 255, 38, 39], [255] * 4]
    out, skipped = R.gather(src, [1, 10, 2 ** 40], dst, 0, skip_out_of_range=True)
    assert skipped == 2 and out[0].tolist() == [4, 5, 6, 7] and (out[1:] == 255).all()


# ------------------------------------------------------------------------------------------------------------------- host-only entry points

def _error(call):
    with pytest.raises(PastureError) as e:
        call()
    return e.value.code


def _empty(hip, attrs=(A.POSITION_3D,), kind=HashMapBuffer):
    return kind.new_from_layout(PointLayout.from_attributes(list(attrs), api=hip))


def test_kernel_shape(hip):
    assert alg.reorder_kernel_shape(hip) == {"points_per_block": PPB, "record_tile_bytes": TILE_BYTES}
    one = C.c_uint32(7)
    hip.reorder_kernel_shape(None, C.byref(one))  # each pointer is optional
    assert one.value == TILE_BYTES
    hip.reorder_kernel_shape(None, None)
    assert _error(lambda: hip.reorder_phase_times(None)) == 1
    assert len(alg.reorder_phase_times(hip)) == 3


def test_argument_errors_answered_on_the_host(hip):
    """Every listed argument error, with the same status with or without a device: no device is looked for before them."""
    fake, fake2 = C.c_void_p(8), C.c_void_p(4096)  # never dereferenced: every call below is answered before that
    a, b = _empty(hip), _empty(hip, kind=VectorBuffer)
    other = _empty(hip, (A.POSITION_3D, A.INTENSITY))
    # gathers -- 1: null arguments and the index width
    assert _error(lambda: hip.buffer_gather(None, fake, 32, 1, 1, b._h, 0)) == 1
    assert _error(lambda: hip.buffer_gather(a._h, fake, 32, 1, 1, None, 0)) == 1
    assert _error(lambda: hip.buffer_gather(a._h, None, 32, 1, 1, b._h, 0)) == 1
    assert _error(lambda: hip.buffer_gather(a._h, fake, 32, 9, 1, b._h, 0)) == 1
    for bits in (0, 8, 16, 33, 128):
        assert _error(lambda: hip.buffer_gather(a._h, fake, bits, 1, 1, b._h, 0)) == 1
        assert _error(lambda: hip.buffer_gather_async(a._h, fake, bits, 1, b._h, 0, None)) == 1
        assert _error(lambda: hip.buffer_take(a._h, fake, bits, 1, 1, 0, C.byref(C.c_void_p()))) == 1
    assert _error(lambda: hip.buffer_gather_async(None, fake, 32, 1, b._h, 0, None)) == 1
    assert _error(lambda: hip.buffer_gather_async(a._h, None, 64, 1, b._h, 0, None)) == 1
    assert _error(lambda: hip.buffer_take(a._h, fake, 32, 1, 1, 0, None)) == 1
    assert _error(lambda: hip.buffer_take(None, fake, 32, 1, 1, 0, C.byref(C.c_void_p()))) == 1
    assert _error(lambda: hip.buffer_take(a._h, fake, 32, 1, 1, 2, C.byref(C.c_void_p()))) == 1
    assert _error(lambda: hip.buffer_take(a._h, None, 32, 1, 1, 0, C.byref(C.c_void_p()))) == 1
    # 2: the layouts differ -- before the range; a bad index width before the layouts
    assert _error(lambda: hip.buffer_gather(a._h, fake, 32, 1, 1, other._h, 0)) == 2
    assert _error(lambda: hip.buffer_gather_async(a._h, fake, 64, 1, other._h, 0, None)) == 2
    assert _error(lambda: hip.buffer_gather(a._h, fake, 7, 1, 1, other._h, 0)) == 1
    with pytest.raises(PasturePanic):
        hip.buffer_gather(a._h, fake, 32, 1, 0, other._h, 0)
    # 5: dst_first + count beyond dst
    assert _error(lambda: hip.buffer_gather(a._h, fake, 32, 1, 1, b._h, 0)) == 3
    assert _error(lambda: hip.buffer_gather(a._h, fake, 32, 1, 0, b._h, 1)) == 3
    assert _error(lambda: hip.buffer_gather_async(a._h, fake, 32, 2 ** 63, b._h, 2 ** 63, None)) == 3
    # count == 0 and empty buffers: answered on the host
    hip.buffer_gather(a._h, None, 32, 1, 0, b._h, 0)
    hip.buffer_gather_async(a._h, None, 64, 0, b._h, 0, None)
    out = a.take(np.zeros(0, dtype=np.uint32))
    assert out.len() == 0 and isinstance(out, HashMapBuffer) and a.take(np.zeros(0, dtype=np.int64), VectorBuffer).len() == 0
    with pytest.raises(ValueError):
        a.take(np.array([-1]))
    with pytest.raises(TypeError):
        a.take(np.array([1.0]))
    with pytest.raises(TypeError):
        a.gather_into_async(b, np.zeros(3, dtype=np.uint32))

    # sort order by attribute
    f64, pos = T.F64.to_c(), T.Vec3f64.to_c()
    g = _empty(hip, (A.POSITION_3D, A.GPS_TIME))
    assert _error(lambda: hip.sort_order_by_attribute_device(None, b"GpsTime", C.byref(f64), 0, 0, fake)) == 1
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, None, C.byref(f64), 0, 0, fake)) == 1
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"GpsTime", None, 0, 0, fake)) == 1
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"GpsTime", C.byref(f64), 0, 0, None)) == 1
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"GpsTime", C.byref(f64), 1, 0, fake)) == 1
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"Position3D", C.byref(pos), 3, 0, fake)) == 1
    for opaque in (T.ByteArray(8), T.Custom(8, 8, b"0123456789abcdef"), T.Vec4u8):
        cdt = opaque.to_c()
        h = _empty(hip, (Def.custom("Thing", opaque),))
        assert _error(lambda: hip.sort_order_by_attribute_device(h._h, b"Thing", C.byref(cdt), 0, 0, fake)) == 1
    f32 = T.F32.to_c()
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"GpsTime", C.byref(f32), 0, 0, fake)) == 4  # by name AND datatype
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"Intensity", C.byref(f64), 0, 0, fake)) == 4
    assert _error(lambda: hip.sort_order_by_attribute_device(g._h, b"Intensity", C.byref(f64), 1, 0, fake)) == 1  # the component first
    hip.sort_order_by_attribute_device(g._h, b"GpsTime", C.byref(f64), 0, 1, fake)  # empty: nothing to write
    assert alg.argsort_attribute(g, A.GPS_TIME).shape == (0,)

    # Morton order
    assert _error(lambda: hip.morton_order_device(None, 3, 0, fake, None)) == 1
    assert _error(lambda: hip.morton_order_device(a._h, 3, 0, None, None)) == 1
    for dims in (0, 1, 4):
        assert _error(lambda: hip.morton_order_device(a._h, dims, 1, fake, None)) == 1
    assert _error(lambda: hip.morton_order_device(a._h, 3, 22, fake, None)) == 1
    assert _error(lambda: hip.morton_order_device(a._h, 2, 32, fake, None)) == 1
    v3f32 = _empty(hip, (A.POSITION_3D.with_custom_datatype(T.Vec3f32),))
    assert _error(lambda: hip.morton_order_device(v3f32._h, 3, 0, fake, None)) == 4
    assert _error(lambda: hip.morton_order_device(v3f32._h, 5, 0, fake, None)) == 1
    no_position = _empty(hip, (A.INTENSITY,))
    assert _error(lambda: hip.morton_order_device(no_position._h, 2, 31, fake, None)) == 4
    hip.morton_order_device(a._h, 2, 31, fake, None)
    hip.morton_order_device(a._h, 3, 21, fake, fake2)
    order, keys = alg.morton_order(a, return_keys=True)
    assert order.shape == (0,) and keys.shape == (0,) and keys.dtype == np.uint64

    # shuffle, invert
    assert _error(lambda: hip.shuffle_order_device(5, 0, None)) == 1
    hip.shuffle_order_device(0, 0, None)
    assert _error(lambda: hip.invert_order_device(None, 5, fake)) == 1
    assert _error(lambda: hip.invert_order_device(fake, 5, None)) == 1
    assert _error(lambda: hip.invert_order_device(fake, 5, fake)) == 1  # no in-place inversion
    hip.invert_order_device(None, 0, None)
    assert alg.shuffle_order(0, 3, api=hip).shape == (0,)


def test_no_cpu_fallback_without_device(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    fake, fake2 = C.c_void_p(8), C.c_void_p(4096)
    for call in (lambda: hip.shuffle_order_device(5, 1, fake),
                 lambda: hip.invert_order_device(fake, 5, fake2),
                 lambda: _empty(hip).take(np.zeros(3, dtype=np.uint32)),
                 lambda: _empty(hip, kind=VectorBuffer).take(np.zeros(3, dtype=np.int64), HashMapBuffer),
                 lambda: alg.shuffle_order(7, 0, api=hip)):
        with pytest.raises(PastureError) as e:
            call()
        assert e.value.code == 21


# ------------------------------------------------------------------------------------------------------------------------------ GPU: gather

@pytest.mark.gpu
@pytest.mark.parametrize("dst_kind", ["V", "H"])
@pytest.mark.parametrize("src_kind", ["V", "H"])
@pytest.mark.parametrize("layout_name", ["xyz", "las", "las_packed", "blob5"])
def test_gather_every_length_and_pattern(hip, layout_name, src_kind, dst_kind):
    assert alg.reorder_kernel_shape(hip) == {"points_per_block": PPB, "record_tile_bytes": TILE_BYTES}
    layout = layout_of(layout_name, hip)
    mask = written_bytes(layout, src_kind, dst_kind)
    rng = np.random.default_rng(11)
    case = 0
    for n in LENGTHS:
        src_rec = records(layout, n, 100 + n)
        src = filled(src_kind, layout, src_rec)
        src_rec = all_records(src)  # (a columnar buffer has no padding bytes to keep)
        for name, idx in index_patterns(n, rng):
            count = len(idx)
            dst = filled(dst_kind, layout, records(layout, count + 5, 7 * n + count))
            before = all_records(dst)
            what, keep = index_forms(idx, case)
            first = case % 3 if count else 0
            src.gather_into(dst, what, first)
            want = R.gather(src_rec, idx, before, first, mask)
            got = all_records(dst)
            assert np.array_equal(got, want), f"{layout_name} {src_kind}->{dst_kind} n {n} {name} form {case % 5}: rows {np.flatnonzero((got != want).any(axis=1))[:8]}"
            case += 1


@pytest.mark.gpu
@pytest.mark.parametrize("src_kind,dst_kind", [("V", "V"), ("V", "H"), ("H", "V"), ("H", "H")])
def test_gather_records_larger_than_the_tile(hip, src_kind, dst_kind):
    """ByteArray(12000) at 70 points: not even 16 records fit the LDS record tile, the byte-copy kernel takes them"""
    layout = layout_of("blob12k", hip)
    assert 16 * layout.size_of_point_entry() > TILE_BYTES
    src = filled(src_kind, layout, records(layout, 70, 1))
    src_rec = all_records(src)
    rng = np.random.default_rng(2)
    for case, (name, idx) in enumerate(index_patterns(70, rng)):
        dst = filled(dst_kind, layout, records(layout, len(idx) + 2, 3 + case))
        before = all_records(dst)
        what, keep = index_forms(idx, case)
        src.gather_into(dst, what, 1)
        assert np.array_equal(all_records(dst), R.gather(src_rec, idx, before, 1, written_bytes(layout, src_kind, dst_kind))), name


@pytest.mark.gpu
@pytest.mark.parametrize("src_kind,dst_kind", [("V", "V"), ("V", "H"), ("H", "V"), ("H", "H")])
def test_gather_more_attributes_than_one_launch_takes(hip, src_kind, dst_kind):
    """110 attributes of 1, 2, 4 and 8 bytes with padding between them: the attribute table of a launch holds fewer, the gather takes several"""
    kinds = [T.U8, T.U16, T.U32, T.F64, T.I8]
    layout = PointLayout.from_attributes([Def.custom(f"A{i}", kinds[i % 5]) for i in range(110)], api=hip)
    assert not R.attribute_byte_mask(layout).all()
    n = PPB + 9
    src = filled(src_kind, layout, records(layout, n, 1))
    rng = np.random.default_rng(2)
    for case, idx in enumerate((rng.integers(0, n, 2 * n), np.concatenate([rng.integers(0, n, 40), [n + 5], rng.integers(0, n, 300)]))):
        dst = filled(dst_kind, layout, records(layout, len(idx) + 1, 3))
        before = all_records(dst)
        mask = written_bytes(layout, src_kind, dst_kind)
        if case == 0:
            src.gather_into(dst, idx, 1)
            want = R.gather(all_records(src), idx, before, 1, mask)
        else:  # the skipped entry is counted once, not once per launch
            import torch
            skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
            d = DeviceIndices(idx, 64)
            src.gather_into_async(dst, d.triple, 1, skipped.data_ptr())
            hip.stream_synchronize()
            assert int(skipped.item()) == 1
            want, _ = R.gather(all_records(src), idx, before, 1, mask, skip_out_of_range=True)
        assert np.array_equal(all_records(dst), want)


@pytest.mark.gpu
@pytest.mark.parametrize("src_kind,dst_kind", [("V", "V"), ("V", "H"), ("H", "V"), ("H", "H")])
def test_gather_slices_and_a_target_window(hip, src_kind, dst_kind):
    """A slice as source, a slice and dst_first > 0 as target: bytes outside [dst_first, dst_first + count) of the target are unchanged"""
    layout = layout_of("las_packed", hip)
    mask = written_bytes(layout, src_kind, dst_kind)
    rng = np.random.default_rng(5)
    whole_src = filled(src_kind, layout, records(layout, 2 * PPB + 40, 1))
    src = whole_src.slice(range(13, 13 + PPB + 20))
    src_rec = all_records(whole_src)[13:13 + PPB + 20]
    whole_dst = filled(dst_kind, layout, records(layout, 3 * PPB, 2))
    for case, (s0, s1, first, count) in enumerate([(7, 3 * PPB - 9, 5, PPB + 1), (1, 100, 0, 99), (PPB, 2 * PPB + 3, 3, PPB - 2), (0, 3 * PPB, 2 * PPB, 1)]):
        before = all_records(whole_dst)
        idx = rng.integers(0, len(src_rec), count)
        what, keep = index_forms(idx, case + 1)
        src.gather_into(whole_dst.slice(range(s0, s1)), what, first)
        want = before.copy()
        want[s0:s1] = R.gather(src_rec, idx, before[s0:s1], first, mask)
        assert np.array_equal(want[:s0 + first], before[:s0 + first]) and np.array_equal(want[s0 + first + count:], before[s0 + first + count:])
        assert np.array_equal(all_records(whole_dst), want), (s0, s1, first, count)
    # disjoint slices of ONE buffer are a legal pair; overlapping ones are not
    one = filled(src_kind, layout, records(layout, 300, 3))
    before = all_records(one)
    idx = rng.integers(0, 100, 150)
    one.slice(range(0, 100)).gather_into(one.slice(range(100, 300)), idx, 20)
    want = before.copy()
    want[100:] = R.gather(before[:100], idx, before[100:], 20, written_bytes(layout, src_kind, src_kind))
    assert np.array_equal(all_records(one), want)
    for lo in (0, 50, 99):
        assert _error(lambda: one.slice(range(0, 100)).gather_into(one.slice(range(lo, 300)), idx[:10])) == 1
    assert _error(lambda: one.gather_into(one, idx[:10])) == 1
    assert np.array_equal(all_records(one), want)


@pytest.mark.gpu
def test_gather_external_memory_at_an_odd_base(hip):
    import torch
    layout = layout_of("las_packed", hip)
    size = layout.size_of_point_entry()
    n = PPB + 37
    rec = records(layout, n, 4)
    mem = torch.zeros(n * size + 1, dtype=torch.uint8, device="cuda")
    mem[1:] = torch.from_numpy(rec.reshape(-1)).cuda()
    ext = ExternalMemoryBuffer(mem[1:], layout)
    assert ext.points_ptr() % 2 == 1
    idx = np.random.default_rng(6).integers(0, n, 2 * n + 1)
    for kind in ("V", "H"):  # out of external memory ...
        dst = filled(kind, layout, records(layout, len(idx), 5))
        before = all_records(dst)
        ext.gather_into(dst, idx)
        assert np.array_equal(all_records(dst), R.gather(rec, idx, before, 0, written_bytes(layout, "V", kind)))
    for kind in ("V", "H"):  # ... and into it
        src = filled(kind, layout, records(layout, n, 8))
        before = mem.cpu().numpy().copy()
        sel = idx[:n - 3]
        src.gather_into(ext, sel.astype(np.uint32), 2)
        want = before.copy()
        want[1:] = R.gather(all_records(src), sel, before[1:].reshape(n, size), 2, written_bytes(layout, kind, "V")).reshape(-1)
        assert np.array_equal(mem.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("src_kind,dst_kind", [("V", "V"), ("V", "H"), ("H", "V"), ("H", "H")])
@pytest.mark.parametrize("layout_name", ["las", "blob12k"])
def test_out_of_range_indices(hip, layout_name, src_kind, dst_kind):
    """Synchronous: status 3 and the target byte-identical.  Stream-ordered: every valid point written, the others left, the exact count."""
    import torch
    layout = layout_of(layout_name, hip)
    n = 70 if layout_name == "blob12k" else 2 * PPB + 9
    src = filled(src_kind, layout, records(layout, n, 1))
    src_rec = all_records(src)
    rng = np.random.default_rng(3)
    for case, bits in enumerate((32, 64)):
        idx = rng.integers(0, n, n + 11).astype(np.uint64)
        bad = rng.random(len(idx)) < 0.2
        bad[[0, len(idx) - 1]] = True
        idx[bad] = rng.integers(n, 2 ** 32 - 1, int(bad.sum()))
        if bits == 64:
            idx[0] = 2 ** 63 + 5
        idx[1] = n  # the first index that is out of range
        dst = filled(dst_kind, layout, records(layout, len(idx) + 3, 9))
        before = all_records(dst)
        d = DeviceIndices(idx, bits)
        for what in (idx.astype(np.uint32 if bits == 32 else np.uint64), d.triple):
            assert _error(lambda: src.gather_into(dst, what, 2)) == 3
            assert np.array_equal(all_records(dst), before)
        with pytest.raises(PasturePanic):
            src.take(idx.astype(np.uint32 if bits == 32 else np.uint64))
        skipped = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        src.gather_into_async(dst, d.triple, 2, skipped.data_ptr())
        hip.stream_synchronize()
        wrapped = idx if bits == 64 else idx.astype(np.uint32)
        want, n_skipped = R.gather(src_rec, wrapped, before, 2, written_bytes(layout, src_kind, dst_kind), skip_out_of_range=True)
        assert int(skipped.item()) == n_skipped == int((wrapped >= n).sum()) > 0
        assert np.array_equal(all_records(dst), want)
    # the other errors, with a device present: layouts, overlap (above), range
    other = filled(dst_kind, layout_of("xyz", hip), records(layout_of("xyz", hip), 4, 1))
    assert _error(lambda: src.gather_into(other, np.arange(2))) == 2
    small = filled(dst_kind, layout, records(layout, 4, 1))
    assert _error(lambda: src.gather_into(small, np.arange(5))) == 3
    assert _error(lambda: src.gather_into(small, np.arange(3), 2)) == 3
    src.gather_into(small, np.arange(2), 2)
    skipped = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    src.gather_into_async(small, (0, 0, 32), 0, skipped.data_ptr())  # an empty list: the count is still written
    hip.stream_synchronize()
    assert int(skipped.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout_name", ["xyz", "las", "blob5"])
def test_take_equals_gather_and_filter(hip, layout_name):
    layout = layout_of(layout_name, hip)
    n = 3 * PPB + 17
    rng = np.random.default_rng(8)
    for src_kind in ("V", "H"):
        src = filled(src_kind, layout, records(layout, n, 2))
        idx = rng.integers(0, n, n // 2)
        for out_kind in ("V", "H"):
            fresh = KINDS[out_kind].new_from_layout(layout)
            fresh.resize(len(idx))
            before = all_records(fresh)
            src.gather_into(fresh, idx)
            taken = src.take(idx, KINDS[out_kind])
            assert isinstance(taken, KINDS[out_kind]) and taken.len() == len(idx)
            mask = R.attribute_byte_mask(layout)
            assert np.array_equal(all_records(taken)[:, mask], all_records(fresh)[:, mask])
            assert np.array_equal(all_records(fresh), R.gather(all_records(src), idx, before, 0, written_bytes(layout, src_kind, out_kind)))
        assert type(src.take(idx[:5])) is KINDS[src_kind]
        d = DeviceIndices(idx, 32)
        assert np.array_equal(all_records(src.take(d.triple)), all_records(src.take(idx.astype(np.uint64))))
    # an ascending list is a compaction: take(flatnonzero(mask)) is filter(mask)
    src = filled("H", layout, records(layout, n, 3))
    for p in (0.0, 0.3, 1.0):
        keep = rng.random(n) < p
        for out_kind in ("V", "H"):
            a, b = src.take(np.flatnonzero(keep), KINDS[out_kind]), src.filter(KINDS[out_kind], keep)
            assert a.len() == b.len() == int(keep.sum())
            assert np.array_equal(all_records(a), all_records(b))


# ------------------------------------------------------------------------------------------------------------------------- GPU: sort orders

def value_buffer(hip, kind, attribute, values, with_position=True):
    """`values` as the attribute of a buffer (behind a Position3D, so that an interleaved record has a stride)"""
    attrs = ([A.POSITION_3D] if with_position and attribute.name() != "Position3D" else []) + [attribute]
    buf = KINDS[kind].new_from_layout(PointLayout.from_attributes(attrs, api=hip))
    n = len(values)
    if n:
        buf.resize(n)
        buf.set_attribute_range(attribute, range(0, n), values)
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCALARS))
def test_argsort_every_scalar_type(hip, name):
    attribute = Def.custom("Value", SCALARS[name])
    dtype = SCALARS[name].numpy_dtype()
    case = 0
    for n in LENGTHS + [BIG]:
        v = special_values(dtype, n, 40 + n)
        for descending in (False, True):
            kind = "VH"[case % 2]
            case += 1
            buf = value_buffer(hip, kind, attribute, v)
            got = alg.argsort_attribute(buf, attribute, 0, descending)
            assert got.dtype == np.uint32 and np.array_equal(got, R.argsort_attribute(v, descending)), (name, n, descending, kind)
            if n == 3 * PPB + 17:  # a sliced buffer, and the order left in device memory
                import torch
                part = buf.slice(range(5, n - 9))
                assert np.array_equal(alg.argsort_attribute(part, attribute, 0, descending), R.argsort_attribute(v[5:n - 9], descending))
                out = torch.zeros(n, dtype=torch.int32, device="cuda")
                assert alg.argsort_attribute(buf, attribute, 0, descending, device_order_ptr=out.data_ptr()) is None
                assert np.array_equal(out.cpu().numpy().view(np.uint32), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name,datatype", [("Vec3f64", T.Vec3f64), ("Vec3f32", T.Vec3f32)])
def test_argsort_vec3_components(hip, name, datatype):
    attribute = Def.custom("Position3D" if name == "Vec3f64" else "Normal", datatype)
    case = 0
    for n in (1, 65, PPB + 1, 3 * PPB + 17, 20_011):
        v = np.stack([special_values(datatype.numpy_dtype(), n, 60 + c) for c in range(3)], axis=1)
        for component in range(3):
            for descending in (False, True):
                buf = value_buffer(hip, "VH"[case % 2], attribute, v)
                case += 1
                got = alg.argsort_attribute(buf, attribute, component, descending)
                assert np.array_equal(got, R.argsort_attribute(np.ascontiguousarray(v[:, component]), descending)), (name, n, component, descending)
                if n == PPB + 1:
                    assert np.array_equal(alg.argsort_attribute(buf.slice(range(3, n)), attribute, component, descending),
                                          R.argsort_attribute(np.ascontiguousarray(v[3:, component]), descending))


@pytest.mark.gpu
def test_argsort_heavy_ties_is_stable(hip):
    """u8 Classification with five classes: within a class the points keep their input order, in both directions"""
    rng = np.random.default_rng(12)
    for n in (3 * PPB + 17, BIG):
        v = rng.integers(0, 5, n).astype(np.uint8)
        for kind in ("V", "H"):
            buf = value_buffer(hip, kind, A.CLASSIFICATION, v)
            for descending in (False, True):
                order = alg.argsort_attribute(buf, A.CLASSIFICATION, descending=descending).astype(np.int64)
                assert np.array_equal(order, R.argsort_attribute(v, descending))
                for c in range(5):
                    assert (np.diff(order[v[order] == c]) > 0).all()


def morton_clouds():
    rng = np.random.default_rng(20)
    n = 3 * PPB + 17
    box = rng.random((n, 3)) * np.array([100.0, 50.0, 10.0]) + np.array([5e5, 5.4e6, 100.0])
    lattice = np.array([(x, y, z) for x in range(8) for y in range(8) for z in range(8)], dtype=np.float64)
    lattice = np.concatenate([lattice, lattice[rng.permutation(512)], lattice])  # every key three times
    one = np.tile(np.array([[3.0, -4.0, 5.0]]), (PPB + 1, 1))
    flat = rng.random((n, 3))
    flat[:, 1] = 7.25  # all of one axis equal
    face = rng.random((n, 3))
    face[rng.random(n) < 0.3, 0] = 1.0  # on the max face
    face[rng.random(n) < 0.3, 2] = 1.0
    face[:3] = [[0, 0, 0], [1, 1, 1], [1, 0, 1]]
    holes = box.copy()
    bad = rng.random(n) < 0.2
    holes[bad, rng.integers(0, 3, int(bad.sum()))] = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, int(bad.sum()))]
    nothing = np.full((PPB + 3, 3), np.nan)
    nothing[::2, 1] = np.inf
    clouds = {"box": box, "lattice": lattice, "one_point": one, "flat_axis": flat, "max_face": face, "non_finite": holes, "no_finite_point": nothing}
    for m in LENGTHS:
        clouds[f"box_{m}"] = box[:m]
    clouds["big"] = rng.normal(0, 1000, (BIG, 3))
    return clouds


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [2, 3])
def test_morton_order_and_keys(hip, dims):
    from test_outliers import make_buffer
    case = 0
    for name, P in morton_clouds().items():
        for bits in (1, 7, 31 if dims == 2 else 21, 0):
            if name == "big" and bits not in (0, 7):
                continue
            kind = "VH"[case % 2]
            case += 1
            buf = make_buffer(hip, P, kind) if len(P) else _empty(hip, kind=KINDS[kind])
            order, keys = alg.morton_order(buf, dims, bits, return_keys=True)
            want_keys = R.morton_keys(P, dims, bits)
            assert keys.dtype == np.uint64 and np.array_equal(keys, want_keys), (name, dims, bits, kind)
            assert order.dtype == np.uint32 and np.array_equal(order, np.argsort(want_keys, kind="stable")), (name, dims, bits, kind)
            assert np.array_equal(alg.morton_order(buf, dims, bits), order)
    holes = morton_clouds()["non_finite"]
    order = alg.morton_order(make_buffer(hip, holes, "H"), dims).astype(np.int64)
    finite = np.isfinite(holes).all(axis=1)
    m = int(finite.sum())
    assert finite[order[:m]].all() and np.array_equal(order[m:], np.flatnonzero(~finite)), "points that are not finite: last, in input order"
    nothing = morton_clouds()["no_finite_point"]
    assert np.array_equal(alg.morton_order(make_buffer(hip, nothing, "V"), dims), np.arange(len(nothing)))
    # a sliced buffer and a packed record: the position at an odd offset
    P = morton_clouds()["box"]
    assert np.array_equal(alg.morton_order(make_buffer(hip, P, "sliceV"), dims, 9), R.morton_order(P, dims, 9))
    assert np.array_equal(alg.morton_order(make_buffer(hip, P, "external"), dims, 9), R.morton_order(P, dims, 9))


@pytest.mark.gpu
def test_shuffle_and_invert(hip):
    import torch
    for n in LENGTHS + [BIG]:
        for seed in (0, 0xC0FFEE, 2 ** 64 - 1):
            order = alg.shuffle_order(n, seed, api=hip)
            keys = alg.sample_priorities("shuffled", seed, 0, n, api=hip)
            assert order.dtype == np.uint32 and np.array_equal(order, np.argsort(keys, kind="stable")), (n, seed)
            assert np.array_equal(order, R.shuffle_order(n, seed))
            assert np.array_equal(np.sort(order), np.arange(n)), "a permutation"
            inverse = alg.invert_order(order, api=hip)
            assert inverse.dtype == np.uint32 and np.array_equal(inverse[order], np.arange(n))
            assert np.array_equal(inverse, R.invert(order))
    # entries >= n are skipped; the device forms
    order = np.array([2, 7, 0, 0xFFFFFFFF, 1], dtype=np.uint32)
    d_order = torch.from_numpy(order.view(np.int32).copy()).cuda()
    d_inverse = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    assert alg.invert_order((d_order.data_ptr(), 5), device_inverse_ptr=d_inverse.data_ptr(), api=hip) is None
    hip.stream_synchronize()
    assert d_inverse.cpu().tolist() == [2, 4, 0, -7, -7]
    out = torch.zeros(100, dtype=torch.int32, device="cuda")
    assert alg.shuffle_order(100, 5, device_order_ptr=out.data_ptr(), api=hip) is None
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.shuffle_order(100, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["V", "H"])
def test_sorted_buffers_equal_take_of_the_order(hip, kind):
    layout = layout_of("las", hip)
    n = 3 * PPB + 17
    rng = np.random.default_rng(30)
    buf = filled(kind, layout, records(layout, n, 31))
    buf.set_attribute_range(A.POSITION_3D, range(0, n), rng.random((n, 3)) * 100)
    buf.set_attribute_range(A.GPS_TIME, range(0, n), np.round(rng.random(n) * 50))  # ties
    buf.set_attribute_range(A.INTENSITY, range(0, n), rng.integers(0, 40, n).astype(np.uint16))
    mask = R.attribute_byte_mask(layout)

    def same(a, b):
        return a.len() == b.len() and np.array_equal(all_records(a)[:, mask], all_records(b)[:, mask])

    for out_kind in (None, "V", "H"):
        out_type = KINDS[out_kind] if out_kind else None
        for attribute, component, descending in ((A.GPS_TIME, 0, False), (A.INTENSITY, 0, True), (A.POSITION_3D, 2, False)):
            s = alg.sort_by_attribute(buf, attribute, component, descending, out_type)
            assert type(s) is (out_type or KINDS[kind])
            assert same(s, buf.take(alg.argsort_attribute(buf, attribute, component, descending), out_type))
            v = s.view_attribute(attribute)
            v = v[:, component] if v.ndim == 2 else v
            assert (np.diff(v.astype(np.float64)) <= 0).all() if descending else (np.diff(v.astype(np.float64)) >= 0).all()
        m, order = alg.morton_sort(buf, 3, 10, out_type, return_order=True)
        assert np.array_equal(order, alg.morton_order(buf, 3, 10)) and same(m, buf.take(order, out_type))
        assert same(alg.morton_sort(buf, 2, 0, out_type), buf.take(alg.morton_order(buf, 2, 0), out_type))
        assert same(alg.shuffle(buf, 77, out_type), buf.take(alg.shuffle_order(n, 77, api=hip), out_type))
    # two calls write the same bytes
    for f in (lambda: alg.morton_sort(buf, 3, 0), lambda: alg.shuffle(buf, 5), lambda: alg.sort_by_attribute(buf, A.GPS_TIME, descending=True)):
        assert np.array_equal(all_records(f()), all_records(f()))
    assert alg.sort_by_attribute(_empty(hip, (A.POSITION_3D, A.GPS_TIME), KINDS[kind]), A.GPS_TIME).len() == 0
    assert alg.morton_sort(_empty(hip, kind=KINDS[kind])).len() == 0 and alg.shuffle(_empty(hip, kind=KINDS[kind]), 1).len() == 0


@pytest.mark.gpu
def test_normals_on_the_morton_sorted_cloud_carry_back(hip):
    """compute_normals on morton_sort(buf), carried back with invert_order, finds the same neighbour SETS as on buf: 20 000 uniform random
    points, no exact ties among the distances"""
    from test_outliers import make_buffer
    n, k = 20_000, 8
    P = np.random.default_rng(40).random((n, 3))
    buf = make_buffer(hip, P, "H")
    _, _, knn = alg.compute_normals(buf, k, return_knn=True)
    sorted_buf, order = alg.morton_sort(buf, return_order=True)
    assert np.array_equal(sorted_buf.view_attribute(A.POSITION_3D), P[order])
    _, _, knn_sorted = alg.compute_normals(sorted_buf, k, return_knn=True)
    inverse = alg.invert_order(order, api=hip).astype(np.int64)
    carried = order.astype(np.int64)[knn_sorted[inverse]]  # row i: the neighbours of original point i, as original indices
    assert np.array_equal(np.sort(carried, axis=1), np.sort(knn, axis=1))
