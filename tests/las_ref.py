"""The LAS point records restated in numpy from the record tables of the LAS 1.4 specification (ASPRS LAS 1.4 R15, tables 7-17: point data
record formats 0-10) -- test helper, numpy only.  Nothing here comes from pasture_amd.las's converters or mapping tables, nor from the oracle:
the reference that the seam tests (test_las_seams.py) hold the device kernels against shares no shift, mask or field order with them.

  decode(raw_bytes, fmt, scale, offset)   raw records -> the named columns of the format's typed layout
  encode(columns, fmt, scale, offset)     the inverse (the LAS writer: truncation toward zero, checked narrowing to i32)
  typed_records / typed_columns           the packed typed record = the columns side by side, and back
  header_bounds / return_counts           what a write adds to the LAS header

Every operation is an IEEE operation that numpy repeats exactly: positions are X.astype(f64) * scale + offset (two roundings, no fused
multiply-add), everything else is bits.  The tests at the end pin this file on the CPU: the 22 fixture files against the literal vectors of
las_expected.py, encode(decode(x)) == x, and random bytes against the oracle.
"""
import os
import struct

import numpy as np
import pytest

import las_expected as E
from minmax_ref import las_header_ref

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
RAW_SIZES = [20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67]

# ---- the eleven raw record dtypes, field by field (little endian, packed) --------------------------------------------------------------------
_XYZ = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4")]
_GPS = [("gps_time", "<f8")]
_RGB = [("red", "<u2"), ("green", "<u2"), ("blue", "<u2")]
_NIR = [("nir", "<u2")]
_WAVE = [("wave_packet_descriptor_index", "u1"), ("byte_offset_to_waveform_data", "<u8"), ("waveform_packet_size", "<u4"),
         ("return_point_waveform_location", "<f4"), ("parametric_dx", "<f4"), ("parametric_dy", "<f4"), ("parametric_dz", "<f4")]
# formats 0-5: one flag byte (return number 3 bits, number of returns 3 bits, scan direction, edge of flight line), then classification,
# scan angle RANK (i8), user data, point source id
_LEGACY = _XYZ + [("intensity", "<u2"), ("flags", "u1"), ("classification", "u1"), ("scan_angle_rank", "i1"), ("user_data", "u1"),
                  ("point_source_id", "<u2")]
# formats 6-10: two flag bytes (return number 4 bits, number of returns 4 bits; classification flags 4 bits, scanner channel 2 bits, scan
# direction, edge of flight line), then classification, USER DATA, scan angle (i16), point source id, GPS time (always)
_EXTENDED = _XYZ + [("intensity", "<u2"), ("flags0", "u1"), ("flags1", "u1"), ("classification", "u1"), ("user_data", "u1"),
                    ("scan_angle", "<i2"), ("point_source_id", "<u2")] + _GPS
RAW_FIELDS = {
    0: _LEGACY,
    1: _LEGACY + _GPS,
    2: _LEGACY + _RGB,
    3: _LEGACY + _GPS + _RGB,
    4: _LEGACY + _GPS + _WAVE,
    5: _LEGACY + _GPS + _RGB + _WAVE,
    6: _EXTENDED,
    7: _EXTENDED + _RGB,
    8: _EXTENDED + _RGB + _NIR,
    9: _EXTENDED + _WAVE,
    10: _EXTENDED + _RGB + _NIR + _WAVE,
}
RAW_DTYPES = {f: np.dtype(fields) for f, fields in RAW_FIELDS.items()}
assert [RAW_DTYPES[f].itemsize for f in range(11)] == RAW_SIZES

# ---- the typed layout: field order written out here, sizes cross-checked against the project's layout by check_typed_layout ------------------
_T_HEAD = [("Position3D", "<f8", (3,)), ("Intensity", "<u2"), ("ReturnNumber", "u1"), ("NumberOfReturns", "u1")]
_T_LEGACY = _T_HEAD + [("ScanDirectionFlag", "u1"), ("EdgeOfFlightLine", "u1"), ("Classification", "u1"), ("ScanAngleRank", "i1"), ("UserData", "u1"),
                       ("PointSourceID", "<u2")]
_T_EXTENDED = _T_HEAD + [("ClassificationFlags", "u1"), ("ScannerChannel", "u1"), ("ScanDirectionFlag", "u1"), ("EdgeOfFlightLine", "u1"),
                         ("Classification", "u1"), ("UserData", "u1"), ("ScanAngle", "<i2"), ("PointSourceID", "<u2"), ("GpsTime", "<f8")]
_T_GPS = [("GpsTime", "<f8")]
_T_RGB = [("ColorRGB", "<u2", (3,))]
_T_NIR = [("NIR", "<u2")]
_T_WAVE = [("WavePacketDescriptorIndex", "u1"), ("WaveformDataOffset", "<u8"), ("WaveformPacketSize", "<u4"), ("ReturnPointWaveformLocation", "<f4"),
           ("WaveformParameters", "<f4", (3,))]
TYPED_FIELDS = {
    0: _T_LEGACY,
    1: _T_LEGACY + _T_GPS,
    2: _T_LEGACY + _T_RGB,
    3: _T_LEGACY + _T_GPS + _T_RGB,
    4: _T_LEGACY + _T_GPS + _T_WAVE,
    5: _T_LEGACY + _T_GPS + _T_RGB + _T_WAVE,
    6: _T_EXTENDED,
    7: _T_EXTENDED + _T_RGB,
    8: _T_EXTENDED + _T_RGB + _T_NIR,
    9: _T_EXTENDED + _T_WAVE,
    10: _T_EXTENDED + _T_RGB + _T_NIR + _T_WAVE,
}
TYPED_DTYPES = {f: np.dtype(fields) for f, fields in TYPED_FIELDS.items()}
TYPED_ORDER = {f: [x[0] for x in fields] for f, fields in TYPED_FIELDS.items()}
TYPED_SIZES = [TYPED_DTYPES[f].itemsize for f in range(11)]


def check_typed_layout(layout, fmt):
    """The project's typed layout of the format has the field order, offsets and size written out above."""
    dt = layout.numpy_record_dtype()
    assert list(dt.names) == TYPED_ORDER[fmt], (fmt, dt.names)
    mine = TYPED_DTYPES[fmt]
    assert dt.itemsize == mine.itemsize and [dt.fields[k][1] for k in dt.names] == [mine.fields[k][1] for k in mine.names], (fmt, dt, mine)
    assert [dt.fields[k][0].itemsize for k in dt.names] == [mine.fields[k][0].itemsize for k in mine.names], (fmt, dt, mine)


def _records(raw_bytes, fmt):
    raw = np.ascontiguousarray(raw_bytes, dtype=np.uint8).reshape(-1, RAW_SIZES[fmt])
    return np.frombuffer(raw.tobytes(), dtype=RAW_DTYPES[fmt]) if raw.shape[0] else np.zeros(0, dtype=RAW_DTYPES[fmt])


def decode(raw_bytes, fmt, scale, offset):
    """Raw records (n x record size bytes) -> {attribute name: column} in the typed layout's order."""
    r = _records(raw_bytes, fmt)
    c = {}
    # two roundings per component: RN(RN(X * scale) + offset)
    c["Position3D"] = np.stack([r[a].astype(np.float64) * np.float64(scale[k]) + np.float64(offset[k]) for k, a in enumerate("XYZ")], axis=1)
    c["Intensity"] = r["intensity"].copy()
    if fmt <= 5:
        f = r["flags"]
        c["ReturnNumber"] = f & 7
        c["NumberOfReturns"] = f >> 3 & 7
        c["ScanDirectionFlag"] = f >> 6 & 1
        c["EdgeOfFlightLine"] = f >> 7
        c["Classification"] = r["classification"].copy()
        c["ScanAngleRank"] = r["scan_angle_rank"].copy()
        c["UserData"] = r["user_data"].copy()
    else:
        f0, f1 = r["flags0"], r["flags1"]
        c["ReturnNumber"] = f0 & 15
        c["NumberOfReturns"] = f0 >> 4
        c["ClassificationFlags"] = f1 & 15
        c["ScannerChannel"] = f1 >> 4 & 3
        c["ScanDirectionFlag"] = f1 >> 6 & 1
        c["EdgeOfFlightLine"] = f1 >> 7
        c["Classification"] = r["classification"].copy()
        c["UserData"] = r["user_data"].copy()
        c["ScanAngle"] = r["scan_angle"].copy()
    c["PointSourceID"] = r["point_source_id"].copy()
    names = r.dtype.names
    if "gps_time" in names:
        c["GpsTime"] = r["gps_time"].copy()  # bits: NaN payloads stay
    if "red" in names:
        c["ColorRGB"] = np.stack([r["red"], r["green"], r["blue"]], axis=1)
    if "nir" in names:
        c["NIR"] = r["nir"].copy()
    if "waveform_packet_size" in names:
        c["WavePacketDescriptorIndex"] = r["wave_packet_descriptor_index"].copy()
        c["WaveformDataOffset"] = r["byte_offset_to_waveform_data"].copy()
        c["WaveformPacketSize"] = r["waveform_packet_size"].copy()
        c["ReturnPointWaveformLocation"] = r["return_point_waveform_location"].copy()
        # three f32 moved as u32 and viewed back: np.stack of float arrays could quieten a signalling NaN on some hosts
        c["WaveformParameters"] = np.stack([r[k].view(np.uint32) for k in ("parametric_dx", "parametric_dy", "parametric_dz")], axis=1).view(np.float32)
    assert list(c) == TYPED_ORDER[fmt]
    return {k: np.ascontiguousarray(v) for k, v in c.items()}


def typed_records(columns, fmt):
    """The packed typed records (n x typed size bytes): the columns side by side."""
    assert list(columns) == TYPED_ORDER[fmt]
    n = len(columns["Intensity"])
    rec = np.zeros(n, dtype=TYPED_DTYPES[fmt])
    img = rec.view(np.uint8).reshape(n, -1)
    for k in TYPED_ORDER[fmt]:  # bytes, not values: float fields keep their NaN payloads
        dt, off = TYPED_DTYPES[fmt].fields[k][:2]
        col = np.ascontiguousarray(columns[k])
        assert col.dtype == dt.base and col.nbytes == n * dt.itemsize, (k, col.dtype, dt)
        img[:, off:off + dt.itemsize] = col.view(np.uint8).reshape(n, dt.itemsize)
    return img


def typed_columns(record_bytes, fmt):
    """The inverse of typed_records."""
    img = np.ascontiguousarray(record_bytes, dtype=np.uint8).reshape(-1, TYPED_SIZES[fmt])
    n = img.shape[0]
    out = {}
    for k in TYPED_ORDER[fmt]:
        dt, off = TYPED_DTYPES[fmt].fields[k][:2]
        base = dt.base
        col = np.ascontiguousarray(img[:, off:off + dt.itemsize]).view(base)
        out[k] = col.reshape(n, -1) if dt.shape else col.reshape(n)
    return out


def field_at(fmt, byte, typed=True):
    """Name of the field that holds byte `byte` of a typed (or raw) record: for failure messages."""
    dt = TYPED_DTYPES[fmt] if typed else RAW_DTYPES[fmt]
    for k in dt.names:
        f, off = dt.fields[k][:2]
        if off <= byte < off + f.itemsize:
            return k
    return "?"


def encode(columns, fmt, scale, offset):
    """Typed columns -> raw records (n x record size bytes).  X = trunc((p - offset) / scale) toward zero through i64, which must fit an
    i32 (ValueError otherwise: the writer panics there); flags are packed from the low bits of their columns; the rest is copied."""
    n = len(columns["Intensity"])
    r = np.zeros(n, dtype=RAW_DTYPES[fmt])
    pos = columns["Position3D"]
    for k, a in enumerate("XYZ"):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            local = (pos[:, k] - np.float64(offset[k])) / np.float64(scale[k])
        t = np.trunc(np.where(np.isnan(local), 0.0, local))  # NaN as i64 is 0
        if np.any((t > INT32_MAX) | (t < INT32_MIN)):
            raise ValueError("position out of bounds for this LAS offset and scale")
        r[a] = t.astype(np.int64).astype(np.int32)
    r["intensity"] = columns["Intensity"]
    rn, nr = columns["ReturnNumber"], columns["NumberOfReturns"]
    sd, eof = columns["ScanDirectionFlag"], columns["EdgeOfFlightLine"]
    if fmt <= 5:
        r["flags"] = (rn & 7) | ((nr & 7) << 3) | ((sd & 1) << 6) | ((eof & 1) << 7)
        r["scan_angle_rank"] = columns["ScanAngleRank"]
    else:
        cf, sc = columns["ClassificationFlags"], columns["ScannerChannel"]
        r["flags0"] = (rn & 15) | ((nr & 15) << 4)
        r["flags1"] = (cf & 15) | ((sc & 3) << 4) | ((sd & 1) << 6) | ((eof & 1) << 7)
        r["scan_angle"] = columns["ScanAngle"]
    r["classification"] = columns["Classification"]
    r["user_data"] = columns["UserData"]
    r["point_source_id"] = columns["PointSourceID"]
    img = r.view(np.uint8).reshape(n, -1)

    def put_bits(field, col):  # float fields as bytes
        f, off = RAW_DTYPES[fmt].fields[field][:2]
        img[:, off:off + f.itemsize] = np.ascontiguousarray(col).view(np.uint8).reshape(n, f.itemsize)

    names = r.dtype.names
    if "gps_time" in names:
        put_bits("gps_time", columns["GpsTime"])
    if "red" in names:
        for k, a in enumerate(("red", "green", "blue")):
            r[a] = columns["ColorRGB"][:, k]
    if "nir" in names:
        r["nir"] = columns["NIR"]
    if "waveform_packet_size" in names:
        r["wave_packet_descriptor_index"] = columns["WavePacketDescriptorIndex"]
        r["byte_offset_to_waveform_data"] = columns["WaveformDataOffset"]
        r["waveform_packet_size"] = columns["WaveformPacketSize"]
        put_bits("return_point_waveform_location", columns["ReturnPointWaveformLocation"])
        wp = np.ascontiguousarray(columns["WaveformParameters"]).view(np.uint32).reshape(n, 3)
        for k, a in enumerate(("parametric_dx", "parametric_dy", "parametric_dz")):
            put_bits(a, np.ascontiguousarray(wp[:, k]))
    return img


def encode_typed_records(rec, fmt, scale, offset):
    """encode() of a structured array of typed records (the layout's numpy_record_dtype)."""
    assert list(rec.dtype.names) == TYPED_ORDER[fmt]
    return encode({k: np.ascontiguousarray(rec[k]) for k in TYPED_ORDER[fmt]}, fmt, scale, offset)


def numpy_encode(rec, fmt, scale, offset):
    """The name test_las_encode.py has always used."""
    return encode_typed_records(rec, fmt, scale, offset)


def header_bounds(columns, seeds=None):
    """What a write makes of the header's {min xyz}, {max xyz}: sequential strict compares from the seeds, the first of equal values stays."""
    return las_header_ref(columns["Position3D"], seeds)


def return_counts(columns, max_return):
    """Points per return number 1..max_return (the header's points-by-return): the column's value, not its low bits."""
    return [int(x) for x in np.bincount(columns["ReturnNumber"], minlength=256)[1:max_return + 1]]


def slice_columns(columns, a, b):
    return {k: v[a:b] for k, v in columns.items()}


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "las")


def read_fixture(path):
    """(format, record length, (n, record length) bytes, scale, offset) of an uncompressed .las file: public header block offsets of the
    specification (header size 94, offset to point data 96, format 104, record length 105, legacy count 107, scale / offset 131, count 247)."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"LASF"
    offset_to_points = struct.unpack_from("<I", raw, 96)[0]
    fmt = raw[104] & 0x3F
    rec_len = struct.unpack_from("<H", raw, 105)[0]
    n = struct.unpack_from("<I", raw, 107)[0]
    if raw[25] >= 4 and n == 0:
        n = struct.unpack_from("<Q", raw, 247)[0]
    v = struct.unpack_from("<6d", raw, 131)
    recs = np.frombuffer(raw, dtype=np.uint8, count=n * rec_len, offset=offset_to_points).reshape(n, rec_len).copy()
    return fmt, rec_len, recs, v[:3], v[3:]


FIXTURES = [(f, extra) for f in range(11) for extra in (False, True)]


def _expected_columns(fmt):
    ext = fmt >= 6
    c = {"Position3D": E.POSITIONS, "Intensity": E.INTENSITIES, "ReturnNumber": E.RETURN_NUMBERS_EXTENDED if ext else E.RETURN_NUMBERS,
         "NumberOfReturns": E.NUMBER_OF_RETURNS_EXTENDED if ext else E.NUMBER_OF_RETURNS, "ClassificationFlags": E.CLASSIFICATION_FLAGS,
         "ScannerChannel": E.SCANNER_CHANNELS, "ScanDirectionFlag": E.SCAN_DIRECTION_FLAGS, "EdgeOfFlightLine": E.EDGE_OF_FLIGHT_LINES,
         "Classification": E.CLASSIFICATIONS, "ScanAngleRank": E.SCAN_ANGLE_RANKS, "ScanAngle": E.SCAN_ANGLES_EXTENDED, "UserData": E.USER_DATA,
         "PointSourceID": E.POINT_SOURCE_IDS, "GpsTime": E.GPS_TIMES, "ColorRGB": E.COLORS, "NIR": E.NIRS, "WavePacketDescriptorIndex": E.WAVEPACKET_INDEX,
         "WaveformDataOffset": E.WAVEPACKET_OFFSET, "WaveformPacketSize": E.WAVEPACKET_SIZE, "ReturnPointWaveformLocation": E.WAVEPACKET_LOCATION,
         "WaveformParameters": E.WAVEPACKET_PARAMETERS}
    return {k: c[k] for k in TYPED_ORDER[fmt]}


@pytest.mark.parametrize("fmt,extra", FIXTURES)
def test_reference_decodes_the_fixtures_to_the_literal_vectors(fmt, extra):
    f, rec_len, recs, scale, offset = read_fixture(os.path.join(GOLDEN, f"10_points{'_with_extra_bytes' if extra else ''}_format_{fmt}.las"))
    assert f == fmt and rec_len == RAW_SIZES[fmt] + (4 if extra else 0) and recs.shape[0] == E.N
    got = decode(recs[:, :RAW_SIZES[fmt]], fmt, scale, offset)
    want = _expected_columns(fmt)
    for k in TYPED_ORDER[fmt]:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    if extra:  # the u32 "TestExtraBytes" after the record
        assert np.array_equal(np.ascontiguousarray(recs[:, RAW_SIZES[fmt]:]).view("<u4").reshape(-1), np.arange(E.N, dtype=np.uint32))


@pytest.mark.parametrize("fmt,extra", FIXTURES)
def test_reference_encode_of_decode_reproduces_the_fixture_bytes(fmt, extra):
    _, _, recs, scale, offset = read_fixture(os.path.join(GOLDEN, f"10_points{'_with_extra_bytes' if extra else ''}_format_{fmt}.las"))
    raw = recs[:, :RAW_SIZES[fmt]]
    cols = decode(raw, fmt, scale, offset)
    assert np.array_equal(encode(cols, fmt, scale, offset), raw)
    assert np.array_equal(encode(typed_columns(typed_records(cols, fmt), fmt), fmt, scale, offset), raw)
    mn, mx = header_bounds(cols)
    assert (tuple(mn), tuple(mx)) == E.BOUNDS
    assert return_counts(cols, 15) == [int((cols["ReturnNumber"] == r).sum()) for r in range(1, 16)]


@pytest.mark.parametrize("target_kind", ["V", "H"])
@pytest.mark.parametrize("fmt", range(11))
def test_reference_equals_the_oracle_on_random_bytes(oracle, fmt, target_kind):
    """The production reader's plan run by the oracle on uniformly random record bytes (every field takes every bit pattern) gives the bytes
    of this file's decode; a disagreement here is a finding about pasture_amd/las.py or the oracle."""
    from harness import BUFFER_KINDS
    from pasture_amd import las
    from pasture_amd.buffers import VectorBuffer
    n = 1537
    raw = np.random.default_rng(4200 + fmt).integers(0, 256, size=(n, RAW_SIZES[fmt]), dtype=np.uint8)
    raw_layout = las.point_layout_from_las_point_format(las.Format(fmt), True, api=oracle)
    typed_layout = las.point_layout_from_las_point_format(las.Format(fmt), False, api=oracle)
    check_typed_layout(typed_layout, fmt)
    assert raw_layout.size_of_point_entry() == RAW_SIZES[fmt]
    for scale, offset in (((0.001, 0.001, 0.001), (500000.0, 5400000.0, 100.0)), ((0.01, 0.25, 1.0 / 3.0), (0.0, -0.0, 1e-300)), ((-0.5, 0.125, -1e-3), (-0.0, 7.0, 0.0))):
        dst = BUFFER_KINDS[target_kind].new_from_layout(typed_layout)
        dst.resize(n)
        las.get_default_las_converter(raw_layout, typed_layout, scale, offset).convert_into(VectorBuffer.from_numpy(raw, raw_layout), dst)
        got = dst.get_point_range(range(0, n))
        want = typed_records(decode(raw, fmt, scale, offset), fmt)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (fmt, scale, bad[0], field_at(fmt, int(bad[0][1])))
