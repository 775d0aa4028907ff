"""Bounds and minmax bit for bit: the sign of a zero bound and the bits of a NaN bound.

The reference folds in index order with strict compares, so a bound of +-0 has the sign of the FIRST zero of its component (min([+0, -0]) = +0,
min([-0, +0]) = -0) and a NaN first value of minmax_attribute keeps its payload (tests/minmax_ref.py restates each rule).  Float `==` sees none of
that; these tests compare bits.  CPU tests pin the oracle to the restatement; GPU tests pin every entry point and kernel family of the HIP path to
both.  The mixed-zero data: x has +0 before -0, y has -0 before +0, z has no zero -- in one wave, in two lanes whose grid-stride order is the
reverse of index order, in different blocks, and (6 * 10^6 points, once per entry point) in different first-level fold groups."""
import ctypes as C

import numpy as np
import pytest

from harness import BUFFER_KINDS
from minmax_ref import F64_MAX, aabb_union, assert_same_aabb, assert_same_bits, bounds_ref, las_header_ref, minmax_ref
from pasture_amd import las
from pasture_amd.algorithms import calculate_bounds, calculate_bounds_async, minmax_attribute
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.conversion import BufferLayoutConverter, Transform, jit_set_mode, last_plan_kinds
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition, PointLayout, attributes as A

SNAN64, QNAN64_PAYLOAD = np.uint64(0x7FF0000000000001), np.uint64(0xFFF8000000001234)
SNAN32, QNAN32_PAYLOAD = np.uint32(0x7F800001), np.uint32(0xFFC01234)


def planted(n, i, j, case, seed=0, dtype=np.float64):
    """(n, 3): case "min" = values in [1, 2) with zeros (a zero is the minimum), "max" = values in (-2, -1] with zeros; x: +0 at i, -0 at j;
    y: -0 at i, +0 at j; z: no zero.  i < j."""
    rng = np.random.default_rng(seed)
    p = 1.0 + rng.random((n, 3))
    if case == "max":
        p = -p
    p[i, 0], p[j, 0] = 0.0, -0.0
    p[i, 1], p[j, 1] = -0.0, 0.0
    return p.astype(dtype)


def check_planted_signs(want, case):
    """The restatement's answer on planted(): x +0, y -0 (a guard on the helper itself)."""
    b = want[0] if case == "min" else want[1]
    assert b[0] == 0 and not np.signbit(b[0]) and b[1] == 0 and np.signbit(b[1]), b


def positions_buffer(api, kind, pts, packed=False, dtype=T.Vec3f64):
    """kind V / H; packed: an Intensity (u16) first, so the position sits at byte offset 2 of a 26-byte record."""
    pos = A.POSITION_3D.with_custom_datatype(dtype)
    layout = PointLayout.from_attributes_packed([A.INTENSITY, pos], 1, api=api) if packed else PointLayout.from_attributes([pos], api=api)
    buf = BUFFER_KINDS[kind].new_from_layout(layout)
    pts = np.asarray(pts, dtype=dtype.numpy_dtype()).reshape(-1, 3)
    buf.resize(pts.shape[0])
    buf.set_attribute_range(pos, range(0, pts.shape[0]), pts)
    return buf


def stride_elements():
    """Elements one grid-stride step of the strided reduction covers (stream.hip reduce_grid(): CUs x 8 blocks of 256)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def placements(n_stride):
    """(i, j, n): one wave; lanes 5 and 2 where j is lane 2's SECOND element (grid-stride order reverses index order); different blocks."""
    return [(3, 40, 4096), (5, n_stride + 2, n_stride + 4096), (100, 300_000, 400_000)]


# ---------------------------------------------------------------------------------------------------------------- the restatement, CPU only

def test_reference_restatement_known_answers():
    z = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731
    assert_same_bits(minmax_ref(z(0.0, -0.0))[0], z(0.0))
    assert_same_bits(minmax_ref(z(-0.0, 0.0))[0], z(-0.0))
    assert_same_bits(minmax_ref(z(-0.0, 0.0))[1], z(-0.0))
    assert_same_bits(minmax_ref(z(-1.0, 0.0, -0.0))[1], z(0.0))
    with pytest.raises(AssertionError):
        assert_same_bits(z(0.0), z(-0.0))
    nan = np.array([QNAN64_PAYLOAD], dtype=np.uint64).view(np.float64)
    v = np.concatenate([nan, z(1.0, -3.0)])
    assert_same_bits(minmax_ref(v)[0], nan)  # NaN first seeds and sticks, payload and all
    assert_same_bits(minmax_ref(z(2.0, np.nan, 1.0))[0], z(1.0))
    b = bounds_ref(np.array([[0.0, -0.0, np.nan], [-0.0, 0.0, np.nan]]))
    assert_same_bits(b[0], z(0.0, -0.0, F64_MAX))
    assert_same_bits(b[1], z(0.0, -0.0, -F64_MAX))
    h = las_header_ref(np.array([[-0.0, 0.0, 1.0]]), [0.0, -0.0, 5.0, -0.0, 0.0, 0.5])  # the header's zeros come first
    assert_same_bits(h[0], z(0.0, -0.0, 1.0))
    assert_same_bits(h[1], z(-0.0, 0.0, 1.0))


def test_union_of_chunk_bounds_in_chunk_order_is_the_whole_fold():
    """update_bounds_in_las_header over chunks == over the whole: fold each chunk from the identities, then AABB::union in chunk order."""
    rng = np.random.default_rng(3)
    for case in ("min", "max"):
        p = planted(5000, 10, 3000, case)
        p[rng.integers(0, 5000, 40), rng.integers(0, 3, 40)] = np.where(rng.random(40) < 0.5, 0.0, -0.0)  # planted ties
        hb = [-0.0, 0.0, F64_MAX, 0.0, -0.0, -F64_MAX]
        acc = (np.array(hb[:3]), np.array(hb[3:]))
        for c0 in range(0, 5000, 1000):
            acc = aabb_union(acc, las_header_ref(p[c0:c0 + 1000]))
        want = las_header_ref(p, hb)
        assert_same_bits(acc[0], want[0])
        assert_same_bits(acc[1], want[1])


# ------------------------------------------------------------------------------------------------------------- the oracle, CPU only

@pytest.mark.parametrize("kind", ["V", "H"])
@pytest.mark.parametrize("case", ["min", "max"])
def test_oracle_bounds_of_mixed_zeros(oracle, kind, case):
    for i, j, n in [(0, 1, 2), (3, 40, 100), (7, 900, 1000)]:
        p = planted(n, i, j, case)
        want = bounds_ref(p)
        check_planted_signs(want, case)
        for packed in (False, True):
            assert_same_aabb(calculate_bounds(positions_buffer(oracle, kind, p, packed)), want, f"{case} {i} {j} packed={packed}")
        p32 = p.astype(np.float32)
        assert_same_aabb(calculate_bounds(positions_buffer(oracle, kind, p32, dtype=T.Vec3f32)), bounds_ref(p32), "Vec3f32")


@pytest.mark.parametrize("kind", ["V", "H"])
def test_oracle_bounds_random_ties_infinities_and_nans(oracle, kind):
    rng = np.random.default_rng(7)
    for n in (1, 17, 5000):
        p = np.round(rng.normal(size=(n, 3)) * 2) / 2  # many ties
        m = rng.random((n, 3))
        p[m < 0.2] = 0.0
        p[m < 0.1] = -0.0
        p[(m > 0.95)] = np.inf
        p[(m > 0.97)] = -np.inf
        p[(m > 0.98)] = np.nan
        assert_same_aabb(calculate_bounds(positions_buffer(oracle, kind, p)), bounds_ref(p), f"n={n}")


MINMAX_TYPES = [T.U8, T.I8, T.U16, T.I16, T.U32, T.I32, T.U64, T.I64, T.F32, T.F64, T.Vec3u8, T.Vec3u16, T.Vec3i32, T.Vec3f32, T.Vec3f64]


def minmax_values(dt, n, seed, first_nan=False):
    """Values of datatype dt (n rows, 1 or 3 components): integer extremes (MIN / MAX of the type) planted late; floats: component 0 has +0
    before -0 (a zero minimum), component 1 -0 before +0 in negatives (a zero maximum), component 2 infinities and later NaNs; first_nan: a
    quiet NaN with a payload first in component 0 and a signalling NaN first in component 1."""
    npd = dt.numpy_dtype()
    nc = dt.num_components()
    rng = np.random.default_rng(seed)
    if npd.kind in "iu":
        info = np.iinfo(npd)
        v = rng.integers(max(info.min, -1000), min(info.max, 1000), size=(n, nc), endpoint=True).astype(npd)
        v[n - 2, 0], v[n - 3, nc - 1] = info.min, info.max
        v[n // 2, 0] = info.min
    else:
        v = (1.0 + rng.random((n, nc))).astype(npd)
        v[n // 3, 0], v[n - 1, 0] = 0.0, -0.0
        if nc == 3:
            v[:, 1] = -v[:, 1]
            v[n // 4, 1], v[n // 2, 1] = -0.0, 0.0
            v[n // 5, 2], v[n // 6, 2], v[n // 7, 2] = np.inf, -np.inf, np.nan
        if first_nan:
            ub = np.uint32 if npd.itemsize == 4 else np.uint64
            v[0, 0] = np.array([QNAN32_PAYLOAD if ub is np.uint32 else QNAN64_PAYLOAD], dtype=ub).view(npd)[0]
            if nc == 3:
                v[0, 1] = np.array([SNAN32 if ub is np.uint32 else SNAN64], dtype=ub).view(npd)[0]
    return v if nc == 3 else v[:, 0]


def minmax_buffer(api, kind, dt, vals):
    """The attribute behind a u16 in a packed layout (an offset of 2 in each record: unaligned for every type wider than 2 bytes)."""
    attr = PointAttributeDefinition("Value", dt)
    layout = PointLayout.from_attributes_packed([A.INTENSITY, attr], 1, api=api)
    buf = BUFFER_KINDS[kind].new_from_layout(layout)
    buf.resize(len(vals))
    buf.set_attribute_range(attr, range(0, len(vals)), vals)
    return buf, attr


def check_minmax(api, kind, dt, vals, msg=""):
    buf, attr = minmax_buffer(api, kind, dt, vals)
    got = minmax_attribute(buf, attr)
    want = minmax_ref(vals)
    assert_same_bits(np.atleast_1d(got[0]), want[0], f"{msg} {dt} min")
    assert_same_bits(np.atleast_1d(got[1]), want[1], f"{msg} {dt} max")


@pytest.mark.parametrize("kind", ["V", "H"])
@pytest.mark.parametrize("dt", MINMAX_TYPES, ids=str)
def test_oracle_minmax_every_datatype(oracle, kind, dt):
    check_minmax(oracle, kind, dt, minmax_values(dt, 3001, 11), "oracle")
    if dt.numpy_dtype().kind == "f":
        check_minmax(oracle, kind, dt, minmax_values(dt, 301, 12, first_nan=True), "oracle NaN first")


def test_oracle_las_header_bounds(oracle):
    typed = las.point_layout_from_las_point_format(las.Format(0), False, api=oracle)
    raw = las.point_layout_from_las_point_format(las.Format(0), True, api=oracle)
    for case in ("min", "max"):
        p = planted(1000, 4, 700, case)
        for hb in (None, [-0.0, 0.0, 9.0, 0.0, -0.0, -9.0]):
            bounds = las_encode(oracle, typed, raw, p, hb)
            assert_same_aabb(bounds, las_header_ref(p, hb), f"{case} header={hb}")


def las_encode(api, typed, raw, pos, hb):
    rec = np.zeros(len(pos), dtype=typed_numpy_dtype(typed))
    rec[A.POSITION_3D.name()] = pos
    src = VectorBuffer.from_numpy(rec, typed)
    dst = VectorBuffer.new_from_layout(raw)
    dst.resize(len(pos))
    bounds, _ = las.encode_points(src, 0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), dst, header_bounds=hb)
    return bounds


def typed_numpy_dtype(layout):
    from harness import random_records
    return random_records(layout, 1, 0).dtype


# ------------------------------------------------------------------------------------------------------------------- the HIP path

def _vs_oracle_and_ref(hip_result, oracle_result, want, msg):
    assert_same_aabb(oracle_result, want, msg + " [oracle]")
    assert_same_aabb(hip_result, want, msg + " [hip]")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["H", "V", "V packed", "H Vec3f32"])
def test_calculate_bounds_zero_placement(hip, oracle, form):
    kind, packed, dtype = form[0], "packed" in form, T.Vec3f32 if "f32" in form else T.Vec3f64
    npd = dtype.numpy_dtype()
    for i, j, n in placements(stride_elements()):
        for case in ("min", "max"):
            p = planted(n, i, j, case, seed=i, dtype=npd)
            want = bounds_ref(p)
            check_planted_signs(want, case)
            got = calculate_bounds(positions_buffer(hip, kind, p, packed, dtype))
            _vs_oracle_and_ref(got, calculate_bounds(positions_buffer(oracle, kind, p, packed, dtype)), want, f"{form} {case} i={i} j={j} n={n}")


@pytest.mark.gpu
def test_calculate_bounds_async_records_and_the_two_level_fold(hip):
    """pst_calculate_bounds_async into device memory: a plain record, and one registered in the {min, -max} form (pst_bounds_record_set_form);
    6 * 10^6 points with the zeros in different first-level fold groups; a captured graph replays the search."""
    import torch
    n = 6_000_000
    for case in ("min", "max"):
        p = planted(n, 1000, 5_500_000, case)
        want = bounds_ref(p)
        buf = positions_buffer(hip, "H", p)
        rec = torch.zeros(6, dtype=torch.float64, device="cuda")
        calculate_bounds_async(buf, rec.data_ptr())
        assert_same_aabb(rec.cpu().numpy(), want, f"async {case}")
        neg = torch.zeros(6, dtype=torch.float64, device="cuda")
        hip.bounds_record_set_form(C.c_void_p(neg.data_ptr()), 1)
        try:
            calculate_bounds_async(buf, neg.data_ptr())
            r = neg.cpu().numpy()
            assert_same_aabb((r[:3], -r[3:]), want, f"{{min, -max}} {case}")
            assert_same_bits(r[3:], -want[1], f"{{min, -max}} {case}: the stored -max")
        finally:
            hip.bounds_record_set_form(C.c_void_p(neg.data_ptr()), 0)
        assert_same_aabb(calculate_bounds(buf), want, f"sync {case}")
    # graph capture: the sign is decided on the device, replay by replay
    small = planted(200_000, 7, 150_000, "min")
    buf = positions_buffer(hip, "H", small)
    rec = torch.zeros(6, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    main = torch.cuda.current_stream().cuda_stream
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    try:
        hip.set_stream(C.c_void_p(side.cuda_stream))
        calculate_bounds_async(buf, rec.data_ptr())  # (the workspace of the capturing stream exists before the capture)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            calculate_bounds_async(buf, rec.data_ptr())
    finally:
        hip.set_stream(C.c_void_p(main))
    rec.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert_same_aabb(rec.cpu().numpy(), bounds_ref(small), "graph replay")
    small[[7, 150_000], 0] = small[[150_000, 7], 0]  # swap the zeros: -0 first in x now
    buf.set_attribute_range(A.POSITION_3D, range(0, len(small)), small)
    g.replay()
    torch.cuda.synchronize()
    want = bounds_ref(small)
    assert np.signbit(want[0][0])
    assert_same_aabb(rec.cpu().numpy(), want, "graph replay after the swap")


def _conversion(api, family, n):
    """(converter, src, dst factory, source positions writer) for a conversion with bounds that takes `family`."""
    pos = A.POSITION_3D
    if family == "stream":  # columns -> columns, Vec3f64, affine with scale 1 and offset -0.0 (keeps both zeros)
        lay = PointLayout.from_attributes([pos], api=api)
        conv = BufferLayoutConverter.for_layouts(lay, lay)
        conv.set_custom_mapping_with_transformation(pos, pos, Transform.affine(T.Vec3f64, (1.0, 1.0, 1.0), (-0.0, -0.0, -0.0)), False)
        return conv, lay, lay, "H", "H", pos
    if family == "column":  # columns -> columns, f32 -> f64 cast
        p32 = pos.with_custom_datatype(T.Vec3f32)
        src_l, dst_l = PointLayout.from_attributes([p32], api=api), PointLayout.from_attributes([pos], api=api)
        conv = BufferLayoutConverter.for_layouts(src_l, dst_l)
        conv.set_custom_mapping(p32, pos)
        return conv, src_l, dst_l, "H", "H", p32
    if family == "direct":  # records too large for a tile
        blob = PointAttributeDefinition("Blob", T.ByteArray(70_001))
        lay = PointLayout.from_attributes_packed([pos, A.INTENSITY, blob], 1, api=api)
        return BufferLayoutConverter.for_layouts(lay, lay), lay, lay, "V", "V", pos
    # records -> columns through the interpreter or the plan-specialised kernels: identity copy of a packed, unaligned position
    src_l = PointLayout.from_attributes_packed([A.INTENSITY, pos, A.GPS_TIME], 1, api=api)
    dst_l = PointLayout.from_attributes([pos, A.INTENSITY], api=api)
    return BufferLayoutConverter.for_layouts(src_l, dst_l), src_l, dst_l, "V", "H", pos


FAMILIES = {"stream": {"stream"}, "column": {"column"}, "interpreted": {"interpreted"}, "specialised": {"static", "jit"}, "direct": {"direct"}}


def _run_family(api, family, p, form):
    import torch
    n = len(p)
    conv, src_l, dst_l, sk, dk, src_attr = _conversion(api, family, n)
    src = BUFFER_KINDS[sk].new_from_layout(src_l)
    src.resize(n)
    src.set_attribute_range(src_attr, range(0, n), p.astype(src_attr.datatype().numpy_dtype()))
    dst = BUFFER_KINDS[dk].new_from_layout(dst_l)
    if form == "range":  # (two points in: the 16-byte phase of the columns stays that of the source, so the stream family still takes it)
        dst.resize(n + 2)
        got = conv.convert_into_with_bounds(src, dst, range(0, n), range(2, n + 2))
    else:
        dst.resize(n)
        if form == "sync":
            got = conv.convert_into_with_bounds(src, dst)
        else:
            rec = torch.zeros(6, dtype=torch.float64, device="cuda")
            conv.convert_into_with_bounds_async(src, dst, rec.data_ptr())
            got = rec.cpu().numpy()
    kinds = set(last_plan_kinds(api))
    return got, kinds


def _oracle_conversion_bounds(oracle, family, p, form):
    conv, src_l, dst_l, sk, dk, src_attr = _conversion(oracle, family, len(p))
    n = len(p)
    src = BUFFER_KINDS[sk].new_from_layout(src_l)
    src.resize(n)
    src.set_attribute_range(src_attr, range(0, n), p.astype(src_attr.datatype().numpy_dtype()))
    dst = BUFFER_KINDS[dk].new_from_layout(dst_l)
    dst.resize(n)
    conv.convert_into(src, dst)
    return calculate_bounds(dst)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_conversion_with_bounds_zero_placement_per_family(hip, oracle, family):
    """convert_into_with_bounds / its ranged form / _async on each family a call with bounds can take (COPY never is: converter.cpp), the
    family asserted through pst_last_plan_kinds."""
    mode = {"interpreted": "off", "specialised": "sync"}.get(family)
    if mode:
        jit_set_mode(mode, hip)
    try:
        cases = [(3, 40, 301)] if family == "direct" else placements(stride_elements())
        for i, j, n in cases:
            for case in ("min", "max"):
                p = planted(n, i, j, case, seed=j)
                want = bounds_ref(p.astype(np.float32).astype(np.float64) if family == "column" else p)
                check_planted_signs(want, case)
                ob = _oracle_conversion_bounds(oracle, family, p, "sync")
                for form in ("sync", "range", "async"):
                    got, kinds = _run_family(hip, family, p, form)
                    assert kinds & FAMILIES[family], (family, form, kinds)
                    _vs_oracle_and_ref(got, ob, want, f"{family} {form} {case} i={i} j={j} n={n}")
            if family != "stream":
                break  # (one placement in the slower families: the fold after them is the same finalize)
    finally:
        if mode:
            jit_set_mode("env", hip)


@pytest.mark.gpu
def test_conversion_with_bounds_two_level_fold_stream(hip):
    """6 * 10^6 points, the zeros in different first-level fold groups (kFoldBlocks = 128, stream.hip), both entry forms."""
    for case in ("min", "max"):
        p = planted(6_000_000, 1000, 5_500_000, case)
        want = bounds_ref(p)
        for form in ("sync", "async"):
            got, kinds = _run_family(hip, "stream", p, form)
            assert "stream" in kinds, kinds
            assert_same_aabb(got, want, f"{case} {form}")


@pytest.mark.gpu
def test_las_encoder_header_bounds(hip, oracle):
    """las.encode_points: zeros of both signs in the positions, a +-0 in header_bounds (it counts as the first element), 6 * 10^6 points once;
    write_records_from in chunks with the two zeros in different chunks."""
    import torch
    typed = {a: las.point_layout_from_las_point_format(las.Format(0), False, api=a) for a in (hip, oracle)}
    raw = {a: las.point_layout_from_las_point_format(las.Format(0), True, api=a) for a in (hip, oracle)}
    for case in ("min", "max"):
        for (i, j, n), hb in [((3, 40, 4096), None), ((100, 300_000, 400_000), None), ((5, 9, 4096), [-0.0, 0.0, 9.0, 0.0, -0.0, -9.0]),
                              ((1000, 5_500_000, 6_000_000), None)]:
            p = planted(n, i, j, case, seed=n)
            want = las_header_ref(p, hb)
            ob = las_encode(oracle, typed[oracle], raw[oracle], p, hb) if n < 1_000_000 else want
            _vs_oracle_and_ref(las_encode(hip, typed[hip], raw[hip], p, hb), ob, want, f"{case} n={n} header={hb}")
        p = planted(5000, 10, 3000, case)
        rec = np.zeros(len(p), dtype=typed_numpy_dtype(typed[hip]))
        rec[A.POSITION_3D.name()] = p
        src = HashMapBuffer.from_numpy(rec, typed[hip])
        out = torch.empty(5000 * raw[hip].size_of_point_entry(), dtype=torch.uint8)
        hb = [F64_MAX] * 3 + [-F64_MAX] * 3
        bounds, _ = las.write_records_from(src, 0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), out, header_bounds=hb, chunk_points=1000)
        assert_same_aabb(bounds, las_header_ref(p, hb), f"chunked {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["V", "H"])
def test_minmax_attribute_every_datatype(hip, oracle, kind):
    """Every scalar and Vec3 datatype with a MinMax impl, unaligned in packed records: integer extremes, +-0 in both orders, +-inf, later
    NaNs; NaN first per component (a payload, a signalling NaN) -- vs the restatement and the oracle."""
    for dt in MINMAX_TYPES:
        vals = minmax_values(dt, 3001, 11)
        check_minmax(hip, kind, dt, vals, "hip")
        check_minmax(oracle, kind, dt, vals, "oracle")
        if dt.numpy_dtype().kind == "f":
            first = minmax_values(dt, 301, 12, first_nan=True)
            check_minmax(hip, kind, dt, first, "hip NaN first")


@pytest.mark.gpu
def test_minmax_attribute_past_the_grid_stride(hip):
    """More elements than one grid-stride step: lanes no longer see their elements in index order."""
    n = stride_elements() + 5000
    for dt in (T.F64, T.Vec3f32, T.Vec3f64, T.I64):
        vals = minmax_values(dt, n, 13)
        if dt.numpy_dtype().kind == "f":  # a second pair of zeros: -0 at lane 2 of the second step, +0 at lane 5 of the first
            c = vals if vals.ndim == 1 else vals[:, 0]
            c[n // 3] = 0.5
            c[n - 1] = 0.5
            c[5], c[stride_elements() + 2] = 0.0, -0.0
        check_minmax(hip, "H", dt, vals, "hip")
