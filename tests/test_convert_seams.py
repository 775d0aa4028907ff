"""BufferLayoutConverter's kernel families at every tile and alignment seam, whole targets byte for byte against tests/convert_ref.py.

One builder (`GROUPS`) serves both halves.  Every case starts from a target that already holds a position-dependent byte pattern (the low byte of
splitmix64 of the byte index), with guard points in front of and behind the target range -- and guard bytes inside the same tensor around an
external-memory buffer --, and the comparison is of everything that was read back: unmapped attributes, repr(C) padding, the neighbours'
shares of a 16-byte line.  The source values are each type's edge_values() behind a block made for the affine cases, padded with random values
to a period coprime to 2 and 3, so that over a few tiles every value meets every lane, quad position, component and tile edge.

  CPU half (no marker): the vectorised cast against rust_as_scalar, the fused / unfused count of every affine case, and convert_ref against the
  oracle on every case -- what makes the reference trustworthy without a GPU;
  GPU half (`gpu`): every case on the HIP library with the family forced by jit_set_mode and asserted through last_plan_kinds.
"""
import itertools
from dataclasses import dataclass
from fractions import Fraction
from typing import Callable, Optional, Tuple

import numpy as np
import pytest

from convert_ref import (RefMapping, apply_transform, convert_ref, convert_values, forgive_nan_payloads, fused_bounds_ref, payload_free_nans, rust_as,
                         target_values)
from pasture_amd import conversion as cv
from pasture_amd.algorithms import calculate_bounds, transform_attribute
from pasture_amd.buffers import ExternalMemoryBuffer, HashMapBuffer, VectorBuffer
from pasture_amd.conversion import BufferLayoutConverter, Transform
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition, PointLayout
from rust_as_ref import edge_values, rust_as_scalar

SCALARS = [T.U8, T.U16, T.U32, T.U64, T.I8, T.I16, T.I32, T.I64, T.F32, T.F64]
GUARD = 3  # points in front of and behind every target range
FRAME = 64  # guard bytes on each side of an external-memory buffer (the tile loads read up to 15 B in front of and 31 B behind a tile)
ODD_BASE = 7  # ... plus these in front: the records start at an odd address (a LAS 1.2 header: 375 % 16)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# layouts, sizes and the restated tile rule
# ---------------------------------------------------------------------------------------------------------------------------------------------
def spec(attrs, packed=True):
    """A layout to be: ((name, datatype), ...) and whether it is packed(1) (else repr(C))."""
    return tuple(attrs), packed


def spec_size(s):
    attrs, packed = s
    if packed:
        return sum(t.size() for _, t in attrs)
    off, align = 0, 1
    for _, t in attrs:
        a = t.min_alignment()
        off = (off + a - 1) // a * a + t.size()
        align = max(align, a)
    return (off + align - 1) // align * align


def make_layout(s, api):
    attrs, packed = s
    defs = [PointAttributeDefinition(n, t) for n, t in attrs]
    layout = PointLayout.from_attributes_packed(defs, 1, api=api) if packed else PointLayout.from_attributes(defs, api=api)
    assert layout.size_of_point_entry() == spec_size(s)
    return layout


def tile_points(pairing, src_stride, dst_stride):
    """pick_tile in pasture_amd/csrc/converter.cpp, restated: about 36 KiB of interleaved records per block, a multiple of 64 points."""
    per_point = (src_stride if pairing[0] == "V" else 0) + (dst_stride if pairing[1] == "V" else 0)
    return min(max(36864 // per_point // 64 * 64, 64), 4096)


def seam_counts(t, compiled=False):
    counts = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 3, 8 * t, 8 * t + 1]  # 8 t: the grid is rounded to a multiple of 8
    if compiled:
        counts += [511, 512, 513, 3 * 256 + 255]
    return sorted(set(counts))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# transformations.  The affine parameters are made so that a fused multiply-add shows: for v = 2^23 + j (j in [512, 640)), s = 1 + 2^-40 and
# o = -2^23 - 2^-17 + 2^-15 the product v * s = v + 2^-17 + j 2^-40 rounds to v + 2^-17 (j 2^-40 < 2^-29 / 2, half an ulp), so the two-rounding
# result is j + 2^-15 exactly -- the midpoint of two f32 values, which rounds to the even one, j -- while the fused result keeps j 2^-40, lies above
# the midpoint and rounds to j + 2^-14.  As f64 the two differ as well.  Scaling s and o by a power of two scales everything exactly: the Vec3
# components get 1, 2 and 1/2 times the pair, three distinct scales and offsets whose exchange changes every value.
# ---------------------------------------------------------------------------------------------------------------------------------------------
AFFINE_J = np.arange(512, 640)
AFFINE_S, AFFINE_O = 1.0 + 2.0 ** -40, -2.0 ** 23 - 2.0 ** -17 + 2.0 ** -15
AFFINE_POW = (1.0, 2.0, 0.5)


def affine(datatype):
    return Transform.affine(datatype, tuple(AFFINE_S * p for p in AFFINE_POW), tuple(AFFINE_O * p for p in AFFINE_POW))


def bits(datatype):
    """A bit-field whose shift + width reaches the type's top bit."""
    shift = {T.U8: 3, T.U16: 5, T.U32: 9, T.U64: 13}[datatype]
    return Transform.bitfield(datatype, shift, (1 << (8 * datatype.size() - shift)) - 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    src: tuple
    dst: tuple
    pairing: str  # source and target storage: V (VectorBuffer), H (HashMapBuffer), E (external memory at an odd base)
    n: int
    maps: Tuple = ()  # (source attribute, target attribute, Transform or None, apply_to_source): custom mappings on top of for_layouts_with_default
    s0: int = GUARD
    t0: int = GUARD
    mode: str = "off"
    kinds: Tuple[str, ...] = ("interpreted",)
    bounds: bool = False
    prepare: Optional[Callable] = None  # (records, case) -> None: plants values in the source records
    seed: int = 1

    def __str__(self):
        return f"{self.name} {self.pairing} n={self.n} s0={self.s0} t0={self.t0} mode={self.mode}"


def splitmix_bytes(count, salt=0):
    """The low byte of splitmix64(byte index + salt)."""
    with np.errstate(over="ignore"):
        z = (np.arange(count, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFF)).astype(np.uint8)


def value_pattern(dt, seed):
    """One period of an attribute's source values: the affine block (floats), edge_values, random values up to a length coprime to 2 and 3."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    parts = [(2.0 ** 23 + AFFINE_J).astype(dt)] if dt.kind == "f" else []
    parts.append(edge_values(dt))
    have = sum(p.size for p in parts)
    extra = next(k for k in range(97, 104) if (have + k) % 6 in (1, 5))
    if dt.kind == "f":
        mags = 10.0 ** rng.uniform(-3, 25 if dt.itemsize == 8 else 20, size=extra)
        with np.errstate(over="ignore"):
            parts.append((mags * rng.choice([-1.0, 1.0], size=extra)).astype(dt))
    else:
        info = np.iinfo(dt)
        parts.append(rng.integers(info.min, info.max, size=extra, dtype=dt, endpoint=True))
    out = np.concatenate(parts)
    assert all(np.gcd(out.size, k) == 1 for k in (3, 4, 64, 256))
    return out


def source_records(case, layout, count):
    """The period starts at the first point of the source range (so the affine block lies in every range that has room for it)."""
    rec = np.zeros(count, dtype=layout.numpy_record_dtype())
    raw = rec.view(np.uint8).reshape(count, -1)
    raw[:] = splitmix_bytes(raw.size, 77).reshape(raw.shape)  # the source's own padding is not zero either
    for i, a in enumerate(layout.attributes()):
        nc = a.datatype().num_components()
        flat = np.roll(np.resize(value_pattern(a.datatype().numpy_dtype(), 1000 * case.seed + i), count * nc), case.s0 * nc)
        rec[a.name()] = flat.reshape(count, nc) if nc > 1 else flat
    if case.prepare is not None:
        case.prepare(rec, case)
    return rec


def make_converter(case, src_l, dst_l):
    conv = BufferLayoutConverter.for_layouts_with_default(src_l, dst_l)
    xfs = {}
    for s_name, t_name, xf, pre in case.maps:
        sd, td = src_l.get_attribute_by_name(s_name).attribute_definition(), dst_l.get_attribute_by_name(t_name).attribute_definition()
        if xf is None:
            conv.set_custom_mapping(sd, td)
        else:
            conv.set_custom_mapping_with_transformation(sd, td, xf, pre)
            xfs[t_name] = (xf, pre)
    maps = []
    for m in conv.mappings():
        xf, pre = xfs.get(m.target.name(), (None, False))
        assert bool(m.transform_kind) == (xf is not None) and m.apply_to_source == pre
        sm, tm = src_l.get_attribute(m.source), dst_l.get_attribute(m.target)
        assert sm.offset() == m.source_offset and tm.offset() == m.target_offset
        maps.append(RefMapping(sm, tm, xf, pre))
    return conv, maps


class Frame:
    """An interleaved or columnar buffer of `count` points holding given bytes, and how to read ALL of it back.  kind E: the records lie at an odd
    address inside a larger device tensor, FRAME guard bytes on each side; read() then checks those guard bytes itself."""

    def __init__(self, kind, layout, content, on_gpu):
        self.kind, self.layout = kind if on_gpu or kind != "E" else "V", layout
        self.count = content.shape[0] if not isinstance(content, dict) else next(iter(content.values())).shape[0]
        if self.kind == "H":
            self.buffer = HashMapBuffer.new_from_layout(layout)
            self.buffer.resize(self.count)
            cols = content if isinstance(content, dict) else {a.name(): content[a.name()] for a in layout.attributes()}
            for a in layout.attributes():
                self.buffer.set_attribute_range(a.attribute_definition(), range(0, self.count), cols[a.name()])
        elif self.kind == "V":
            self.buffer = VectorBuffer.new_from_layout(layout)
            self.buffer.resize(self.count)
            self.buffer.set_point_range(range(0, self.count), np.ascontiguousarray(content))
        else:
            import torch
            raw = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
            self.lead = FRAME + ODD_BASE
            self.frame = splitmix_bytes(self.lead + raw.size + FRAME, 5)
            self.frame[self.lead:self.lead + raw.size] = raw
            self.tensor = torch.from_numpy(self.frame.copy()).cuda()
            inner = self.tensor[self.lead:self.lead + raw.size]
            assert inner.data_ptr() % 2 == 1
            self.buffer = ExternalMemoryBuffer(inner, layout)
            assert self.buffer.len() == self.count

    def read(self):
        if self.kind == "H":
            return {a.name(): self.buffer.view_attribute(a.attribute_definition()) for a in self.layout.attributes()}
        if self.kind == "V":
            return np.ascontiguousarray(self.buffer.get_point_range(range(0, self.count)))
        import torch
        torch.cuda.synchronize()
        got = self.tensor.cpu().numpy()
        size = self.count * self.layout.size_of_point_entry()
        assert np.array_equal(got[:self.lead], self.frame[:self.lead]), "bytes in front of the external buffer changed"
        assert np.array_equal(got[self.lead + size:], self.frame[self.lead + size:]), "bytes behind the external buffer changed"
        return got[self.lead:self.lead + size].reshape(self.count, -1).copy()


def target_prior(kind, layout, count):
    if kind == "H":
        out = {}
        for i, a in enumerate(layout.attributes()):
            nc, dt = a.datatype().num_components(), a.datatype().numpy_dtype()
            col = splitmix_bytes(count * a.size(), 1000003 * (i + 1)).view(dt)
            out[a.name()] = col.reshape(count, nc) if nc > 1 else col
        return out
    return splitmix_bytes(count * layout.size_of_point_entry(), 31).reshape(count, layout.size_of_point_entry())


def assert_same_target(got, want, what):
    if isinstance(want, dict):
        for k in want:
            g, w = np.ascontiguousarray(got[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)
            if not np.array_equal(g, w):
                bad = np.flatnonzero(g != w)
                raise AssertionError(f"{what}: column {k}: {bad.size} bytes differ, first at byte {bad[:8].tolist()} (value size {want[k][0:1].nbytes})")
    else:
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{what}: {bad.shape[0]} bytes differ, first at (point, byte) {bad[:8].tolist()}")


def run_case(case, api, on_gpu):
    """Runs the case on `api` and compares everything read back with convert_ref.  Returns the source records and mappings (for the counts)."""
    src_l, dst_l = make_layout(case.src, api), make_layout(case.dst, api)
    n, s0, t0 = case.n, case.s0, case.t0
    sr, tr = range(s0, s0 + n), range(t0, t0 + n)
    rec = source_records(case, src_l, s0 + n + GUARD)
    conv, maps = make_converter(case, src_l, dst_l)
    src = Frame(case.pairing[0], src_l, rec, on_gpu)
    prior = target_prior("H" if case.pairing[1] == "H" else "V", dst_l, t0 + n + GUARD)
    dst = Frame(case.pairing[1], dst_l, prior, on_gpu)
    want = convert_ref(rec, maps, prior, sr, tr)
    want_bounds = None
    if case.bounds:
        want_bounds = fused_bounds_ref(target_values(want, dst_l.get_attribute_by_name("Position3D"), t0, n))
    if on_gpu:
        cv.jit_set_mode(case.mode, api)
        if case.bounds:
            aabb = conv.convert_into_with_bounds(src.buffer, dst.buffer, sr, tr)
        else:
            conv.convert_into_range(src.buffer, sr, dst.buffer, tr)
        kinds = cv.last_plan_kinds(api)
        assert set(kinds) == set(case.kinds) and len(kinds) == len(case.kinds), f"{case}: took {kinds}, expected {list(case.kinds)}"
    else:
        conv.convert_into_range(src.buffer, sr, dst.buffer, tr)
        aabb = calculate_bounds(dst.buffer.slice(tr)) if case.bounds else None
    got = forgive_nan_payloads(dst.read(), want, payload_free_nans(rec, maps, sr), tr)
    assert_same_target(got, want, str(case))
    src_after = src.read()  # the source is not written, nor what lies around it
    assert_same_target(src_after, {k: rec[k] for k in src_after} if isinstance(src_after, dict) else rec.view(np.uint8).reshape(rec.shape[0], -1),
                       f"{case} (source)")
    if case.bounds:
        got_bounds = np.array(tuple(aabb.min()) + tuple(aabb.max()), dtype=np.float64).view(np.uint64)
        assert np.array_equal(got_bounds, want_bounds), f"{case}: bounds {[hex(int(x)) for x in got_bounds]}, expected {[hex(int(x)) for x in want_bounds]}"
    return rec, maps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fused against unfused, in exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _nearest_f64(q):
    try:
        return float(q)  # int / int true division: correctly rounded
    except OverflowError:
        return float("inf") if q > 0 else float("-inf")


def fused_affine(values, xf):
    """The transformation with ONE rounding to f64, round(v * s + o), then the type's own rounding -- what a contracted kernel computes."""
    v = np.asarray(values)
    out = np.array(apply_transform(v, xf)).reshape(v.shape[0], -1)
    flat = v.reshape(v.shape[0], -1)
    for (i, c), x in np.ndenumerate(flat):
        if np.isfinite(x):
            with np.errstate(over="ignore"):
                out[i, c] = v.dtype.type(_nearest_f64(Fraction(float(x)) * Fraction(xf.scale[c]) + Fraction(xf.offset[c])))
    return out.reshape(v.shape)


def fused_differences(rec, maps, source_range, limit=128):
    """Per affine mapping: how many of the first `limit` points' TARGET values differ between the fused and the two-rounding affine."""
    counts = {}
    n = min(limit, len(source_range))
    for m in maps:
        if m.transform is None or m.transform.kind != cv.XF_AFFINE:
            continue
        v = np.ascontiguousarray(rec[m.source.name()][source_range.start:source_range.start + n])
        tdt = m.target.datatype().numpy_dtype()
        if m.apply_to_source:
            fused = rust_as(fused_affine(v, m.transform), tdt)
        else:
            fused = fused_affine(rust_as(v, tdt), m.transform)
        plain = convert_values(v, m)
        counts[m.target.name()] = (int(np.count_nonzero((fused != plain) & ~(np.isnan(fused) & np.isnan(plain)))), v.size)
    return counts


def assert_fused_differences(case, rec, maps):
    for name, (differ, values) in fused_differences(rec, maps, range(case.s0, case.s0 + case.n)).items():
        # a case of fewer than 64 values cannot hold 64: then every value of it has to differ (the affine block comes first in the range)
        assert differ >= min(64, values), f"{case}: {name}: only {differ} of the first {values} values tell a fused affine from the two roundings"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the layouts
# ---------------------------------------------------------------------------------------------------------------------------------------------
S35 = spec([("Position3D", T.Vec3f64), ("Classification", T.U8), ("Intensity", T.U16), ("GpsTime", T.F64)])
D25 = spec([("GpsTime", T.F64), ("Position3D", T.Vec3f32), ("Classification", T.U32), ("Intensity", T.U8)])  # 35 -> 25: the quad mapping
D32 = spec([("Position3D", T.Vec3f64), ("GpsTime", T.F32), ("Intensity", T.U8), ("Classification", T.U16), ("Classification2", T.U8)])  # a multiple of 32: one point per lane
S32 = spec([("Position3D", T.Vec3f64), ("GpsTime", T.F64)])  # interleaved source of 32 B: one point per lane whatever the target
D18 = spec([("GpsTime", T.F32), ("Position3D", T.Vec3f32), ("Flags", T.U16)])  # 2 mod 4
S30 = spec([("Position3D", T.Vec3f64), ("Intensity", T.U16), ("Time", T.F32)])  # 2 mod 4
D16 = spec([("Position3D", T.Vec3f32), ("Time", T.F32)])  # a multiple of 16
S12 = spec([("A", T.U32), ("B", T.I32), ("C", T.F32)])  # multiples of 4
D20 = spec([("B", T.F64), ("A", T.U64), ("C", T.I32)])
PARTIAL = spec([("Classification", T.U8), ("Extra", T.U32), ("Position3D", T.Vec3f64), ("Intensity", T.U16)], packed=False)  # 40 B: Extra unmapped, 3 + 6 B padding
PAIRS = {"p35_25": (S35, D25, ()), "p35_32": (S35, D32, (("Classification", "Classification2", None, False),)), "p32_18": (S32, D18, (("GpsTime", "Flags", None, False),)),
         "p30_16": (S30, D16, ()), "p12_20": (S12, D20, ())}
assert [spec_size(s) for s in (S35, D25, D32, S32, D18, S30, D16, S12, D20, PARTIAL)] == [35, 25, 32, 32, 18, 30, 16, 12, 20, 40]

CLASS_ATTRS = [("a", T.U8), ("b", T.U16), ("c", T.Vec3u8), ("d", T.U32), ("e", T.Vec3u16), ("f", T.U64), ("g", T.Vec3i32), ("h", T.Vec3f32),
               ("p", T.Vec3f64), ("q", T.Vec4u8), ("r", T.I64)]
CLASS_CHANGED = {"a": T.U32, "b": T.U8, "c": T.Vec3u16, "d": T.U16, "e": T.Vec3u8, "g": T.Vec3f32, "h": T.Vec3i32, "p": T.Vec3f32, "r": T.F32}


def class_specs(k, changed):
    """packed(1) records with ByteArray(k) in front of one attribute of every length, odd stride; the target holds them in reverse order."""
    lead = [("lead", T.ByteArray(k))] if k else []
    src = lead + CLASS_ATTRS
    dst = lead + [(n, CLASS_CHANGED.get(n, t) if changed else t) for n, t in reversed(CLASS_ATTRS)]
    fix = lambda attrs: attrs + ([("tail", T.U8)] if sum(t.size() for _, t in attrs) % 2 == 0 else [])  # noqa: E731
    return spec(fix(src)), spec(fix(dst))


WAVES_SRC = spec([("a", T.U8), ("b", T.U16), ("c", T.U32), ("d", T.I8), ("e", T.I16), ("f", T.F32), ("g", T.Vec3u8), ("h", T.U8), ("p", T.Vec3f64), ("q", T.F64)])
WAVES_DST = spec([("p", T.Vec3f64), ("a", T.U16), ("b", T.U8), ("c", T.U32), ("d", T.I32), ("e", T.I16), ("f", T.F32), ("g", T.Vec3u8), ("h", T.U8), ("q", T.F64)])
MANY_SRC = spec([(f"a{i}", SCALARS[i % 10]) for i in range(31)])
MANY_DST = spec([(f"a{i}", SCALARS[(i + 3) % 10]) for i in reversed(range(31))])  # 31 mappings: more than PST_PLAN_MAX_ENTRIES (30), two launches

XF_SRC = spec([("P64", T.Vec3f64), ("P32", T.Vec3f32), ("f32", T.F32), ("f64", T.F64), ("u8", T.U8), ("u16", T.U16), ("u32", T.U32), ("u64", T.U64), ("i64", T.I64)])
XF_DST = spec([("A", T.Vec3f32), ("B", T.Vec3f32), ("C", T.Vec3f64), ("D", T.Vec3f64), ("E", T.F64), ("F", T.F64), ("G", T.F32), ("H", T.F32),
               ("b1", T.U32), ("b2", T.U16), ("b3", T.U8), ("b4", T.I8), ("c1", T.U64), ("c2", T.U32), ("c3", T.U16), ("c4", T.U8)])
# pre- and post-affine across Vec3f64 <-> Vec3f32 and F32 <-> F64; a bit-field of each unsigned type before a narrowing cast (U8 has nothing narrower:
# to I8) and after one (U64 has nothing wider: from I64)
XF_MAPS = (("P64", "A", affine(T.Vec3f64), True), ("P64", "B", affine(T.Vec3f32), False), ("P32", "C", affine(T.Vec3f32), True), ("P32", "D", affine(T.Vec3f64), False),
           ("f32", "E", affine(T.F32), True), ("f32", "F", affine(T.F64), False), ("f64", "G", affine(T.F64), True), ("f64", "H", affine(T.F32), False),
           ("u64", "b1", bits(T.U64), True), ("u32", "b2", bits(T.U32), True), ("u16", "b3", bits(T.U16), True), ("u8", "b4", bits(T.U8), True),
           ("i64", "c1", bits(T.U64), False), ("u64", "c2", bits(T.U32), False), ("u32", "c3", bits(T.U16), False), ("u16", "c4", bits(T.U8), False))
XF_DST_LANE = spec(XF_DST[0] + (("unmapped", T.ByteArray(9)),))  # 128 B: the one-point-per-lane forms of the same mappings
assert spec_size(XF_SRC) == 71 and spec_size(XF_DST) == 119 and spec_size(XF_DST_LANE) == 128

AS_SRC = spec([(f"s{i}", t) for i, t in enumerate(SCALARS)])


def as_group(g):
    """The 90 scalar pairs dealt into three target layouts of 30 mappings each (one launch: PST_PLAN_MAX_ENTRIES)."""
    pairs = [(i, j) for i, j in itertools.permutations(range(10), 2)][g::3]
    dst = spec([(f"s{i}_t{j}", SCALARS[j]) for i, j in pairs])
    return AS_SRC, dst, tuple((f"s{i}", f"s{i}_t{j}", None, False) for i, j in pairs)


BIG_SRC = spec([("sfill", T.ByteArray(2600)), ("v", T.F64), ("u", T.U16)])  # records too large for a tile (64 of them are beyond the LDS cap)
BIG_DST = spec([("u", T.U16), ("dfill", T.ByteArray(2600)), ("v", T.F32)])
BIG_MAPS = (("u", "u", bits(T.U16), False), ("v", "v", affine(T.F32), False))

COL_WIDE_SRC = spec([("P", T.Vec3f32), ("Q", T.Vec3f64), ("u64", T.U64), ("f", T.F64), ("g", T.F32)])
COL_WIDE_DST = spec([("P", T.Vec3f64), ("Q", T.Vec3f32), ("u64", T.U32), ("f", T.F32), ("g", T.F64)])
COL_WIDE_MAPS = (("P", "P", affine(T.Vec3f32), True), ("Q", "Q", affine(T.Vec3f64), True), ("u64", "u64", bits(T.U64), True), ("f", "f", affine(T.F32), False),
                 ("g", "g", affine(T.F64), False))  # both affine arms, before and after the cast
COL_BYTE_SRC = spec([("b", T.ByteArray(5)), ("u8", T.U8), ("c", T.Vec3u8), ("i8", T.I8)])
COL_BYTE_DST = spec([("b", T.ByteArray(5)), ("u8", T.U8), ("c", T.Vec3u8), ("i8", T.U8)])
COL_BYTE_MAPS = (("u8", "u8", bits(T.U8), False),)

BIG41 = spec([("GpsTime", T.F64), ("ColorRGB", T.Vec3u16), ("Position3D", T.Vec3f64), ("Classification", T.U8), ("Intensity", T.I16)])  # harness.custom_point_type_big
INPLACE_32 = spec([("Position3D", T.Vec3f64), ("Intensity", T.U16), ("Classification", T.U8)], packed=False)  # 27 B of attributes, 5 of padding
INPLACE_8 = spec([("Intensity", T.U16), ("Classification", T.U8), ("Time", T.F32)], packed=False)  # one byte of padding in the middle
BOUNDS_SRC = spec([("Position3D", T.Vec3f32), ("Classification", T.U8), ("Intensity", T.U16)])
BOUNDS_DST = spec([("Intensity", T.U16), ("Position3D", T.Vec3f64), ("Classification", T.U8)])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------------------------------------------------------
PAIRINGS = ("VH", "HV", "VV")


def _t(pairing, src, dst):
    return tile_points(pairing, spec_size(src), spec_size(dst))


def takes_quads(pairing, src, dst):
    """build_plan in converter.cpp: four consecutive points per lane iff dst_stride % 32 != 0 and not (interleaved source with src_stride % 32 == 0)."""
    return spec_size(dst) % 32 != 0 and not (pairing[0] == "V" and spec_size(src) % 32 == 0)


def jit_kinds(n, aligned=True):
    if n < 256 or not aligned:
        return ("interpreted",)
    return ("jit",) if n % 256 == 0 else ("jit", "interpreted")


def interpreted_counts():
    out = []
    for name in ("p35_25", "p35_32"):  # every count, on both lane mappings
        src, dst, maps = PAIRS[name]
        for p in PAIRINGS:
            out += [Case(name, src, dst, p, n, maps) for n in seam_counts(_t(p, src, dst))]
    for name in ("p32_18", "p30_16", "p12_20"):  # the other record sizes around the tile
        src, dst, maps = PAIRS[name]
        for p in PAIRINGS:
            t = _t(p, src, dst)
            out += [Case(name, src, dst, p, n, maps) for n in (t - 1, t, t + 1, 2 * t + 3)]
    return out


def interpreted_starts():
    """(a): an odd stride at sixteen consecutive starts puts the first record at every byte of a 16-byte line; two tiles, so the seam between them moves too."""
    src, dst, maps = PAIRS["p35_25"]
    out = []
    for k in range(16):
        out.append(Case("start", src, dst, "VV", _t("VV", src, dst) + 1, maps, s0=GUARD, t0=GUARD + k))
        out.append(Case("start", src, dst, "VV", _t("VV", src, dst) + 1, maps, s0=k, t0=GUARD))
        out.append(Case("start", src, dst, "HV", _t("HV", src, dst) + 1, maps, s0=1, t0=GUARD + k))
        out.append(Case("start", src, dst, "VH", _t("VH", src, dst) + 1, maps, s0=k, t0=GUARD + 2))
    return out


def interpreted_external():
    src, dst, maps = PAIRS["p35_25"]
    out = []
    for p in ("VE", "HE", "EH", "EV", "EE"):
        t = _t(p.replace("E", "V"), src, dst)
        out += [Case("external", src, dst, p, n, maps) for n in (5, t + 1, 2 * t + 3)]
    return out


def class_cases():
    """(c): every load and store alignment class of every attribute length, as plain copies and with the type changes."""
    out = []
    for changed in (False, True):
        for k in range(4):
            src, dst = class_specs(k, changed)
            for p in PAIRINGS:
                out.append(Case(f"classes{'_as' if changed else ''}_k{k}", src, dst, p, _t(p, src, dst) + 1))
    return out


def waves_and_launches():
    out = []
    for p in PAIRINGS:
        t = _t(p, WAVES_SRC, WAVES_DST)
        out += [Case("waves", WAVES_SRC, WAVES_DST, p, n) for n in (t + 1, 2 * t + 3)]
        out.append(Case("31mappings", MANY_SRC, MANY_DST, p, _t(p, MANY_SRC, MANY_DST) + 1))
    return out


def partial_cases():
    """(f): t0 = 3 puts the target's first record at byte 120 = 7 * 16 + 8."""
    out = []
    for p in PAIRINGS:
        t = _t(p, S35, PARTIAL)
        out += [Case("partial", S35, PARTIAL, p, n) for n in (t + 1, 2 * t + 3)]
    return out


def as_cases():
    return [Case(f"as{g}", *as_group(g)[:2], p, _t(p, *as_group(g)[:2]) + 1, as_group(g)[2]) for g in range(3) for p in PAIRINGS]


def xf_cases():
    out = []
    for name, dst in (("xf", XF_DST), ("xf_lane", XF_DST_LANE)):  # four points per lane, and one
        for p in PAIRINGS:
            t = _t(p, XF_SRC, dst)
            out += [Case(name, XF_SRC, dst, p, n, XF_MAPS) for n in (t + 1, 2 * t + 3)]
    return out


def compiled_plans():
    """At most 16 distinct plans: (c) once as copies and once with the type changes, (f), (h) and one layout of (g), each in the three pairings
    ((f) has no record target in V->H: two), plus the fused-bounds plan below.  Starts of 16 points: every interleaved side and every column
    begins on a 16-byte line."""
    plans = []
    for p in PAIRINGS:
        plans.append(("classes_k1", *class_specs(1, False), (), p))
        plans.append(("classes_as_k3", *class_specs(3, True), (), p))
        plans.append(("xf", XF_SRC, XF_DST, XF_MAPS, p))
        plans.append(("as1", *as_group(1), p))
        if p != "VH":
            plans.append(("partial", S35, PARTIAL, (), p))
    return plans


def compiled_cases(plan):
    name, src, dst, maps, p = plan
    out = [Case(name, src, dst, p, n, maps, s0=16, t0=16, mode="sync", kinds=jit_kinds(n)) for n in seam_counts(_t(p, src, dst), compiled=True)]
    # an unaligned start is not taken by a compiled plan
    out.append(Case(name, src, dst, p, 512, maps, s0=GUARD if p[0] == "V" else 16, t0=GUARD if p[1] == "V" else 16, mode="sync", kinds=("interpreted",)))
    return out


def static_cases():
    out = []
    for p in ("HV", "VH"):
        for n in (256, 3 * 256 + 255, 2048):
            out.append(Case("big41", BIG41, BIG41, p, n, s0=16, t0=16, mode="sync", kinds=("static",) if n % 256 == 0 else ("static", "interpreted")))
    return out


def column_cases():
    out = []
    small = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]
    for name, src, dst, maps, vec in (("col_wide", COL_WIDE_SRC, COL_WIDE_DST, COL_WIDE_MAPS, 2), ("col_byte", COL_BYTE_SRC, COL_BYTE_DST, COL_BYTE_MAPS, 16)):
        # a block of the column kernel moves 256 lanes x 4 accesses x `vec` components of the widest type (columns.hip)
        for n in small + [k * vec for k in (1023, 1024, 1025, 4095, 4096, 4097)]:
            out.append(Case(name, src, dst, "HH", n, maps, s0=1, t0=GUARD + 1, kinds=("column",)))  # the two columns at different 16-byte phases
    for g in range(3):
        src, dst, maps = as_group(g)
        out += [Case(f"as{g}", src, dst, "HH", n, maps, s0=1, t0=GUARD + 2, kinds=("column",)) for n in (257, 2 * 1025)]
    return out


def direct_cases():
    return [Case("big_records", BIG_SRC, BIG_DST, p, n, BIG_MAPS, kinds=("direct",)) for p in PAIRINGS for n in (1, 65, 257, 1000)]


def copy_cases():
    return [Case("identity", S35, S35, "VV", n, s0=s0, t0=t0, kinds=("copy",)) for n in (1, 3, 63, 257, 1000, 4097) for s0, t0 in ((1, 5), (4, 3), (0, 7))]


def _plant_positions(p_index, component, value):
    def prepare(rec, case):
        rng = np.random.default_rng(case.n + p_index)
        rec["Position3D"] = rng.uniform(-1000.0, 1000.0, size=rec["Position3D"].shape).astype(np.float32)
        rec["Position3D"][case.s0 + p_index, component] = value
    return prepare


def _plant_nans(rec, case):
    """NaNs (quiet, signalling, negative) on both sides of each extreme, at the range's ends and across the compiled kernel's last tile edge."""
    rng = np.random.default_rng(case.n)
    pos = rng.uniform(-1000.0, 1000.0, size=rec["Position3D"].shape).astype(np.float32)
    s0, n = case.s0, case.n
    edge = n // 256 * 256
    for c, p in enumerate((1, max(edge - 1, 1), n - 2)):
        pos[s0 + p, c] = 2e6 if c % 2 else -2e6
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    for k, p in enumerate((0, 2, max(edge - 2, 0), min(edge, n - 1), n - 3, n - 1)):
        pos[s0 + p, :] = nans[k % 4]
    rec["Position3D"] = pos


def _plant_zero_tie(rec, case):
    """x: the minimum is a tie of +0.0 (first) and -0.0; y: the maximum a tie of -0.0 (first) and +0.0; z: both ends the same -0.0."""
    rng = np.random.default_rng(case.n)
    pos = rng.uniform(1.0, 1000.0, size=rec["Position3D"].shape).astype(np.float32)
    pos[:, 1] *= -1.0
    pos[:, 2] = -0.0
    s0, n = case.s0, case.n
    pos[s0 + 5 % n, 0], pos[s0 + n - 1, 0] = 0.0, -0.0
    pos[s0 + 6 % n, 1], pos[s0 + n - 2, 1] = -0.0, 0.0
    rec["Position3D"] = pos


def bounds_families():
    return [("VH", "off", lambda n: ("interpreted",), GUARD), ("HV", "off", lambda n: ("interpreted",), GUARD), ("VV", "off", lambda n: ("interpreted",), GUARD),
            ("VH", "sync", jit_kinds, 16), ("HH", "off", lambda n: ("column",), GUARD)]


def bounds_cases(family):
    p, mode, kinds_of, start = family
    out = []
    for n in (3 * 256 + 255, _t(p, BOUNDS_SRC, BOUNDS_DST) + 1 if p != "HH" else 4097):
        edge = n // 256 * 256
        spots = [0, edge - 1, edge, n - 1, 100, 101, 102]  # the range's ends, both sides of the compiled kernel's last tile edge, lanes 36, 37, 38 (0, 1, 2 mod 3)
        for k, spot in enumerate(spots):
            value = -3e6 if k % 2 == 0 else 3e6  # a minimum or a maximum, of each component in turn
            out.append(Case(f"plant{spot}", BOUNDS_SRC, BOUNDS_DST, p, n, s0=start, t0=start, mode=mode, kinds=kinds_of(n), bounds=True,
                            prepare=_plant_positions(spot, k % 3, value)))
        out.append(Case("nans", BOUNDS_SRC, BOUNDS_DST, p, n, s0=start, t0=start, mode=mode, kinds=kinds_of(n), bounds=True, prepare=_plant_nans))
        out.append(Case("zero_tie", BOUNDS_SRC, BOUNDS_DST, p, n, s0=start, t0=start, mode=mode, kinds=kinds_of(n), bounds=True, prepare=_plant_zero_tie))
    return out


GROUPS = {
    "interpreted_counts": interpreted_counts,
    "interpreted_starts": interpreted_starts,
    "interpreted_external": interpreted_external,
    "interpreted_classes": class_cases,
    "interpreted_waves_and_launches": waves_and_launches,
    "interpreted_partial": partial_cases,
    "interpreted_as": as_cases,
    "interpreted_xf": xf_cases,
    "static": static_cases,
    "column": column_cases,
    "direct": direct_cases,
    "copy": copy_cases,
}
GROUPS.update({f"compiled_{plan[0]}_{plan[4]}": (lambda plan=plan: compiled_cases(plan)) for plan in compiled_plans()})
GROUPS.update({f"bounds_{f[0]}_{f[1]}": (lambda f=f: bounds_cases(f)) for f in bounds_families()})
COMPILED_PLANS = len(compiled_plans()) + 1  # + the fused-bounds plan of bounds_VH_sync


def test_the_builder_covers_what_it_promises():
    assert COMPILED_PLANS <= 16
    every = [c for make in GROUPS.values() for c in make()]
    assert max(c.n for c in every) <= 70_000
    assert all(c.t0 >= GUARD for c in every)  # (behind the range: run_case appends GUARD points)
    for c in every:
        if c.mode == "sync":  # a compiled plan is expected exactly where every interleaved side starts on a 16-byte line
            aligned = all((start * spec_size(s)) % 16 == 0 for kind, start, s in zip(c.pairing, (c.s0, c.t0), (c.src, c.dst)) if kind == "V")
            assert aligned == (c.kinds != ("interpreted",) or c.n < 256), str(c)
    quads = {(c.pairing, takes_quads(c.pairing, c.src, c.dst)) for c in GROUPS["interpreted_counts"]()}
    assert quads == {(p, q) for p in PAIRINGS for q in (False, True)}  # both lane mappings in every pairing
    assert {spec_size(c.src) % 2 for c in GROUPS["interpreted_starts"]()} == {1} and {spec_size(c.dst) % 2 for c in GROUPS["interpreted_starts"]()} == {1}
    assert {(c.t0 * 25) % 16 for c in GROUPS["interpreted_starts"]() if c.pairing == "VV"} == set(range(16))  # d_mis
    assert {(c.s0 * 35) % 16 for c in GROUPS["interpreted_starts"]() if c.pairing == "VV"} == set(range(16))  # s_mis
    for k in range(4):
        for changed in (False, True):
            assert all(spec_size(s) % 2 == 1 for s in class_specs(k, changed))
    assert (GUARD * spec_size(PARTIAL)) % 16 != 0
    assert sum(1 for _, t in WAVES_SRC[0] if t.size() <= 4) >= 7 and sum(1 for _, t in WAVES_SRC[0] if t.size() > 4) == 2
    assert len(MANY_DST[0]) == 31
    assert sorted(m[:2] for g in range(3) for m in as_group(g)[2]) == sorted((f"s{i}", f"s{i}_t{j}") for i, j in itertools.permutations(range(10), 2))
    for p in PAIRINGS:  # too large for a tile: 64 records of the interleaved sides are beyond the 160 KiB - 256 B the tile kernels may take
        per_point = (spec_size(BIG_SRC) if p[0] == "V" else 0) + (spec_size(BIG_DST) if p[1] == "V" else 0)
        assert per_point > 2559
    for xf in (affine(T.Vec3f64),):
        assert len(set(xf.scale)) == 3 and len(set(xf.offset)) == 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU half
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from_t,to_t", list(itertools.permutations(SCALARS, 2)), ids=lambda t: str(t))
def test_vectorised_cast_is_rust_as(from_t, to_t):
    sdt, tdt = from_t.numpy_dtype(), to_t.numpy_dtype()
    rng = np.random.default_rng(from_t.kind * 16 + to_t.kind)
    if sdt.kind == "f":
        mags = 10.0 ** rng.uniform(-3, 25 if sdt.itemsize == 8 else 20, size=10_000)
        with np.errstate(over="ignore"):
            rnd = (mags * rng.choice([-1.0, 1.0], size=mags.size)).astype(sdt)
    else:
        info = np.iinfo(sdt)
        rnd = rng.integers(info.min, info.max, size=10_000, dtype=sdt, endpoint=True)
    vals = np.concatenate([edge_values(sdt), rnd])
    got = rust_as(vals, tdt)
    want = np.array([rust_as_scalar(v, sdt, tdt) for v in vals], dtype=tdt)
    assert got.dtype == tdt
    if tdt.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want))
        got, want = np.where(np.isnan(got), 0, got), np.where(np.isnan(want), 0, want)
    assert got.tobytes() == want.tobytes(), f"first mismatch at {np.flatnonzero(got != want)[:5]}"


@pytest.mark.parametrize("group", list(GROUPS))
def test_reference_against_the_oracle(oracle, group):
    """convert_ref against the oracle on every case: whole targets; and every affine case holds values that tell a fused affine from the two roundings."""
    seen = set()
    for case in GROUPS[group]():
        rec, maps = run_case(case, oracle, on_gpu=False)
        key = (case.name, case.pairing, min(case.n, 128))
        if key not in seen:  # (the first 128 points of a range do not depend on its length beyond that)
            seen.add(key)
            assert_fused_differences(case, rec, maps)


def test_in_place_reference_against_the_oracle(oracle):
    for case in inplace_cases():
        rec = run_inplace(case, oracle, on_gpu=False)
        name, layout_spec, attr, xf, n, _ = case
        member = make_layout(layout_spec, oracle).get_attribute_by_name(attr)
        assert_fused_differences(Case(name, layout_spec, layout_spec, "VV", n, s0=0, t0=0), rec, [RefMapping(member, member, xf, False)])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# in place: transform_attribute on padded records
# ---------------------------------------------------------------------------------------------------------------------------------------------
def inplace_cases():
    out = []
    for name, layout, xfs in (("inplace32", INPLACE_32, (("Position3D", affine(T.Vec3f64)), ("Intensity", bits(T.U16)))),
                              ("inplace8", INPLACE_8, (("Time", affine(T.F32)), ("Intensity", bits(T.U16))))):
        t = tile_points("HV", 0, spec_size(layout))  # in place: ONE record tile
        for attr, xf in xfs:
            for n in (t - 1, t, t + 1, 2 * t + 3):
                for kind in ("V", "E"):
                    out.append((name, layout, attr, xf, n, kind))
    return out


def run_inplace(case, api, on_gpu):
    name, layout_spec, attr, xf, n, kind = case
    layout = make_layout(layout_spec, api)
    fake = Case(name, layout_spec, layout_spec, kind + kind, n, s0=0, t0=0)
    rec = source_records(fake, layout, n)
    member = layout.get_attribute_by_name(attr)
    prior = rec.view(np.uint8).reshape(n, -1).copy()
    buf = Frame(kind, layout, prior, on_gpu)
    want = convert_ref(rec, [RefMapping(member, member, xf, False)], prior, range(0, n), range(0, n))
    if on_gpu:
        cv.jit_set_mode("off", api)
        empty = VectorBuffer.new_from_layout(layout)  # a conversion of no points: the families noted so far are forgotten
        BufferLayoutConverter.for_layouts(layout, layout).convert_into_range(empty, range(0, 0), empty, range(0, 0))
        assert cv.last_plan_kinds(api) == []
    transform_attribute(buf.buffer, member.attribute_definition(), xf)
    if on_gpu:
        assert cv.last_plan_kinds(api) == ["interpreted"], (case[0], attr, n, cv.last_plan_kinds(api))
    free = payload_free_nans(rec, [RefMapping(member, member, xf, False)], range(0, n))
    assert_same_target(forgive_nan_payloads(buf.read(), want, free, range(0, n)), want, f"{name} {attr} n={n} {kind}")
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU half
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def jit_mode(hip):
    yield hip
    cv.jit_set_mode("env", hip)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_kernels_against_the_reference(jit_mode, group):
    for case in GROUPS[group]():
        run_case(case, jit_mode, on_gpu=True)


@pytest.mark.gpu
def test_in_place_kernel_against_the_reference(jit_mode):
    for case in inplace_cases():
        run_inplace(case, jit_mode, on_gpu=True)
