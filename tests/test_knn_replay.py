"""The stream-ordered replay of compute_normals (pst_compute_normals_plan_create / pst_compute_normals_into_async, pstk::run_normals_replay)
on clouds the plan was NOT made for, against the oracle.

A plan fixes the grid (frame, box, cell edges), the box kernel's instance and two capacities; a replay runs the pipeline on the stream with
no host round trip.  Points outside the recorded box are clamped into boundary cells and their queries go to the exact search, so a replay
is exact for any data unless the status word says otherwise.  Here every replay is made twice, on two plans made from the same cloud under
the same switches:

  * through tests/knn_hooks.py (pstk::run_normals_replay with all three device outputs): f64 normals, f64 curvature and the neighbour lists,
    the plan's facts (grid, shape, capacities) and, after the replay, its device counters;
  * through the public entry, into caller-owned memory (external buffers over a torch tensor): rows pre-filled with NaN bytes, 4096 bytes
    of 0xAB before and after.

A replay whose status has none of bits 0 - 3 set must give, for ALL n rows: the oracle's lists element for element; normals and curvature
inside the windows of test_gpu_parity._compare_normals; a NORMAL column equal to astype(float32) of the hook's f64 normals and a Curvature
column equal to the hook's, bit for bit.  Every status word equals a Python restatement of knn_replay_status_kernel applied to the hook's
counters and capacities; the guard bands are intact after every replay, the flagged ones included.

The displaced clouds R3 / R4 are shifted by multiples of the plan's cell edge h.  The CPU tests (no device) must build the same clouds, so
h is recorded below (_PLAN_H, read from the facts on an MI355X) and every GPU case asserts that the facts still give that value."""
import contextlib
import types

import numpy as np
import pytest

import test_gpu_parity as gp
from pasture_amd._capi import PastureError
from pasture_amd.buffers import HashMapBuffer, VectorBuffer
from pasture_amd.layout import PointAttributeDataType as T, PointAttributeDefinition, PointLayout, attributes as A

CURV = PointAttributeDefinition("Curvature", T.F64)
GUARD = 4096
N = 100_000

# KNN_STATUS_* (pasture_amd/csrc/normals_host.hpp)
FINITE_COUNT, BOX_CAPACITY, FALLBACK_CAPACITY, OPEN_QUERIES, DEGENERATE = 1, 2, 4, 8, 16

# the cell edge h of plans V and S at k = 16, as the device reported it (KnnFacts.h); the shifts of R3 / R4 are multiples of it
_PLAN_H = {"V": 9.291302625498057, "S": 7.415892132961958}


# ---- the status word, restated -------------------------------------------------------------------------------------------------------------
def status_restatement(c, f):
    """knn_replay_status_kernel (normals.hip) in Python: c = the plan's counters after the replay (n_finite, fb_count, box_count,
    open_count[2], error_count), f = the plan's facts (nf, use_list, list_cap, fb_cap) -> [status, status2[1]]"""
    st = 0
    if c.n_finite != f.nf:
        st |= FINITE_COUNT
    if f.use_list and c.box_count > f.list_cap:  # (a plan without a list passes no box count)
        st |= BOX_CAPACITY
    if c.fb_count > f.fb_cap:
        st |= FALLBACK_CAPACITY
    if c.open_count[0] or c.open_count[1]:
        st |= OPEN_QUERIES
    if c.error_count:
        st |= DEGENERATE
    return [st, int(c.error_count) & 0xFFFFFFFFFFFFFFFF]


def _counters(**kw):
    base = dict(n_finite=1000, fb_count=0, box_count=0, open_count=[0, 0], error_count=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _facts(**kw):
    base = dict(nf=1000, use_list=1, list_cap=50, fb_cap=100)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_status_restatement_one_counter_set_per_bit():
    assert status_restatement(_counters(), _facts()) == [0, 0]
    assert status_restatement(_counters(fb_count=100, box_count=50), _facts()) == [0, 0]  # AT capacity is inside it
    assert status_restatement(_counters(n_finite=999), _facts()) == [FINITE_COUNT, 0]
    assert status_restatement(_counters(n_finite=1001), _facts()) == [FINITE_COUNT, 0]
    assert status_restatement(_counters(box_count=51), _facts()) == [BOX_CAPACITY, 0]
    assert status_restatement(_counters(box_count=51), _facts(use_list=0, list_cap=0)) == [0, 0]  # no list: the count is not looked at
    assert status_restatement(_counters(fb_count=101), _facts()) == [FALLBACK_CAPACITY, 0]
    assert status_restatement(_counters(open_count=[1, 0]), _facts()) == [OPEN_QUERIES, 0]
    assert status_restatement(_counters(open_count=[0, 7]), _facts()) == [OPEN_QUERIES, 0]
    assert status_restatement(_counters(error_count=3), _facts()) == [DEGENERATE, 3]
    assert status_restatement(_counters(n_finite=5, box_count=99, fb_count=999, open_count=[2, 2], error_count=1), _facts()) == [31, 1]


# ---- the clouds ------------------------------------------------------------------------------------------------------------------------------
def _tilted_slab(degrees):
    """test_gpu_parity._host_path_cloud("tilted_slab") (degrees = 30) with the angle as a parameter"""
    p = np.random.default_rng(17).random((70_000, 3)) * np.array([1000.0, 40.0, 10.0])
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.column_stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]])


def _generator(plan, seed, n=N):
    if plan == "T":
        return gp._host_path_cloud("tilted_slab")
    return gp._planned_clouds(seed, n, "volume" if plan.startswith("V") else "surface")


def replay_cloud(plan, which, n=N):
    """The cloud `which` of plan `plan` ("V": volume, "S": surface, "T": tilted slab; plans are made on R0).  R1: another seed of the plan's
    generator; R2: R1 with its rows permuted; R3: R1 shifted by half a cell on every axis (+0.5 h; for plan S -0.5 h: its grid is laid from the
    cloud's minimum corner in whole cells and overhangs the far faces by 1.0, 4.5 and 6.2 units, so a shift of +0.5 h = 3.7 leaves 294 points
    outside, a shift towards the origin 16 913); R4: R1 shifted by 2.5 cells along +x (a slab of
    queries beyond one face, inside the six-shell cap of the exact search); R5: R1 scaled by 1.03 about the box centre (a layer beyond all six
    faces); T31: the slab turned by 31 degrees instead of 30; X3: R1 scaled 3x about the centre (most queries outside)."""
    if which == "R0":
        return _generator(plan, 1, n)
    if which == "T31":
        return _tilted_slab(31.0)
    r1 = _generator(plan, 2, n)
    if which == "R1":
        return r1
    if which == "R2":
        return r1[np.random.default_rng(99).permutation(len(r1))]
    if which == "R3":  # (plan S: towards the origin -- see the docstring)
        return r1 + (-0.5 if plan == "S" else 0.5) * _PLAN_H[plan]
    if which == "R4":
        return r1 + np.array([2.5 * _PLAN_H[plan], 0.0, 0.0])
    r0 = _generator(plan, 1, n)
    centre = 0.5 * (r0.min(axis=0) + r0.max(axis=0))
    if which == "R5":
        return centre + 1.03 * (r1 - centre)
    if which == "X3":
        return centre + 3.0 * (r1 - centre)
    raise ValueError(which)


_ORACLE = {}  # (plan, which, n, k) -> the oracle's (normals, curvature, lists): computed once, shared, never modified


def oracle_of(oracle, plan, which, k, n=N):
    key = (plan, which, n, k)
    if key not in _ORACLE:
        pts = replay_cloud(plan, which, n)
        buf = HashMapBuffer.new_from_layout(PointLayout.from_attributes([A.POSITION_3D], api=oracle))
        buf.resize(len(pts))
        buf.set_attribute_range(A.POSITION_3D, range(0, len(pts)), pts)
        from pasture_amd.algorithms import compute_normals
        _ORACLE[key] = compute_normals(buf, k, return_knn=True)
    return _ORACLE[key]


# every (plan, cloud, k) the GPU cases below compare with the oracle: the CPU test pins each of them as free of ties
_STATUS0 = [("V", w) for w in ("R0", "R1", "R2", "R3", "R4", "R5")] + [("S", w) for w in ("R0", "R1", "R2", "R3", "R4", "R5")] + [("T", "R0"), ("T", "T31")]
_OTHER_K = [3, 8, 9, 17, 24, 32, 33, 64]
_COMPARED = [(p, w, 16) for p, w in _STATUS0] + [("V", w, k) for k in _OTHER_K for w in ("R0", "R5")] + [("S", w, 8) for w in ("R0", "R5")]


@pytest.mark.parametrize("plan,which,k", _COMPARED, ids=[f"{p}-{w}-k{k}" for p, w, k in _COMPARED])
def test_replay_clouds_are_free_of_ties(oracle, plan, which, k):
    """The reference of the GPU cases is only unique where no query has its k-th and (k+1)-th neighbour at the same distance: the oracle with
    k + 1 must give d_k < d_(k+1) for every query.  And the reference itself is pinned on the displaced clouds: for 256 queries, among them the
    64 points farthest outside the plan cloud's bounding box, its lists equal a plain float64 brute-force search."""
    pts = replay_cloud(plan, which)
    n = len(pts)
    _, _, ok1 = oracle_of(oracle, plan, which, k + 1)
    assert ok1.shape == (n, k + 1) and ok1.min() >= 0 and ok1.max() < n
    d = ((pts[ok1[:, k - 1:]] - pts[:, None, :]) ** 2).sum(axis=2)  # [n][2]: squared distances of the k-th and (k+1)-th neighbour
    assert (d[:, 0] < d[:, 1]).all(), f"{int((d[:, 0] >= d[:, 1]).sum())} queries with a tie at the k-th neighbour"
    r0 = replay_cloud(plan, "R0")
    beyond = np.maximum(np.maximum(r0.min(axis=0) - pts, pts - r0.max(axis=0)), 0.0).max(axis=1)
    sample = np.unique(np.concatenate([np.argsort(beyond)[-64:], np.random.default_rng(5).choice(n, 192, replace=False)]))
    for first in range(0, len(sample), 64):
        q = sample[first:first + 64]
        d2 = ((pts[None, :, :] - pts[q][:, None, :]) ** 2).sum(axis=2)  # [64][n]
        part = np.argpartition(d2, k + 1, axis=1)[:, :k + 2]  # the k + 2 nearest in no order, then in order
        want = np.take_along_axis(part, np.argsort(np.take_along_axis(d2, part, axis=1), axis=1, kind="stable"), axis=1)[:, :k + 1]
        assert np.array_equal(ok1[q], want), f"the oracle's lists differ from the brute-force search (queries {q[(ok1[q] != want).any(axis=1)][:4].tolist()})"


# ---- plans and replays on the device ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switches(hip, monkeypatch, env):
    from pasture_amd.algorithms import reload_tuning
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    reload_tuning(hip)  # the switches are read once per process
    try:
        yield
    finally:
        monkeypatch.undo()
        reload_tuning(hip)


class _Targets:
    """NORMAL + Curvature in caller-owned device memory, as interleaved records ("records") or as two columns ("columns"): rows of NaN bytes
    between guard bands of 0xAB"""

    def __init__(self, hip, n, kind):
        import torch
        from pasture_amd.buffers import ExternalColumnsBuffer, ExternalMemoryBuffer
        self.n, self.kind = n, kind
        if kind == "records":
            self.layout = PointLayout.from_attributes_packed([A.NORMAL, CURV], 1, api=hip)
            self.stride = self.layout.size_of_point_entry()
            assert self.stride == 20
            self.spans = [(GUARD, n * self.stride)]
        else:
            self.layout = PointLayout.from_attributes([A.NORMAL, CURV], api=hip)
            self.spans = [(GUARD, n * 12), (2 * GUARD + n * 12, n * 8)]
        self.total = self.spans[-1][0] + self.spans[-1][1] + GUARD
        self.t = torch.empty(self.total, dtype=torch.uint8, device="cuda")
        self.reset()
        views = [self.t[o:o + b] for o, b in self.spans]
        self.buf = ExternalMemoryBuffer(views[0], self.layout) if kind == "records" else ExternalColumnsBuffer(views, self.layout, n)

    def reset(self):
        self.t.fill_(0xAB)
        for o, b in self.spans:
            self.t[o:o + b] = 0xFF

    def read(self):
        """-> (NORMAL [n][3] f32, Curvature [n] f64, guard bands intact)"""
        host = self.t.cpu().numpy()
        keep = np.ones(self.total, dtype=bool)
        for o, b in self.spans:
            keep[o:o + b] = False
        intact = bool((host[keep] == 0xAB).all())
        n = self.n
        if self.kind == "records":
            rows = host[GUARD:GUARD + n * self.stride].reshape(n, self.stride)
            offs = {a.name(): a.offset() for a in self.layout.attributes()}
            no, co = offs[A.NORMAL.name()], offs[CURV.name()]
            return rows[:, no:no + 12].copy().view(np.float32).reshape(n, 3), rows[:, co:co + 8].copy().view(np.float64).reshape(n), intact
        (o0, b0), (o1, b1) = self.spans
        return host[o0:o0 + b0].copy().view(np.float32).reshape(n, 3), host[o1:o1 + b1].copy().view(np.float64).reshape(n), intact


class _Plan:
    """Two plans made from ONE cloud under the same switches: one through the hook (facts, counters, all three outputs), one through the
    public entry.  `staged`: the cloud sits in a VectorBuffer of [INTENSITY, POSITION_3D] packed (stride 26), so the plans own a staging copy."""

    def __init__(self, hip, monkeypatch, pts, k, env=None, staged=False):
        import torch
        import knn_hooks
        from pasture_amd.algorithms import NormalsPlan, compute_normals_into
        self.hip, self.k, self.n = hip, k, len(pts)
        self.hooks = knn_hooks.load()
        self.handle = self.public = None
        n = self.n
        self.packed = gp._cloud_buffer(hip, pts)
        self.strided = None
        if staged:
            self.strided = VectorBuffer.new_from_layout(PointLayout.from_attributes_packed([A.INTENSITY, A.POSITION_3D], 1, api=hip))
            self.strided.resize(n)
            self.strided.set_attribute_range(A.POSITION_3D, range(0, n), pts)
        self.normals = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        self.curv = torch.empty(n, dtype=torch.float64, device="cuda")
        self.lists = torch.empty((n, k), dtype=torch.int32, device="cuda")
        self.status = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.records, self.columns = _Targets(hip, n, "records"), _Targets(hip, n, "columns")
        self.sync_want = gp._normal_targets(hip, n)
        with _switches(hip, monkeypatch, env or {}):
            torch.cuda.synchronize()
            pos, stride = self.source(staged)
            rc, rec, valid, why = self.hooks.run_normals(pos, stride, n, k, self.normals.data_ptr(), self.curv.data_ptr(), self.lists.data_ptr())
            try:
                assert rc == 0, rc
                self.valid, self.why_not = valid, why
                if valid:
                    self.handle = self.hooks.plan_create(rec, not staged)
                    assert self.handle, "knn_plan_create failed"
            finally:
                self.hooks.record_free(rec)
            torch.cuda.synchronize()
            if valid:
                self.facts = self.hooks.facts(self.handle)
                self.public = NormalsPlan(self.strided if staged else self.packed, k, gp._normal_targets(hip, n))
                compute_normals_into(self.strided if staged else self.packed, k, self.sync_want)

    def source(self, strided):
        """-> (device address of Position3D of point 0, stride)"""
        if strided:
            off = {a.name(): a.offset() for a in self.strided.point_layout().attributes()}[A.POSITION_3D.name()]
            return self.strided.points_ptr() + off, self.strided.point_layout().size_of_point_entry()
        return self.packed.column_ptr(A.POSITION_3D), 24

    def outside(self, pts):
        """how many of `pts` lie outside the plan's box, from the facts (the grid's frame, origin, cells and cell edges)"""
        f = self.facts
        u = pts
        if f.rotated:
            u = (pts - np.array(f.rot_c[:])) @ np.array(f.rot[:]).reshape(3, 3).T
        org = np.array(f.org[:])
        ext = np.array([f.dim[0] * f.h / f.rx, f.dim[1] * f.h, f.dim[2] * f.h])
        return int(((u < org) | (u >= org + ext)).any(axis=1).sum())

    def replay(self, pts, strided=False):
        """One replay of `pts` through the hook and two through the public entry (records, columns).  Asserts what holds for EVERY replay: the
        status word is the restatement of the counters, the public entry reports the same word, the guard bands are intact.
        -> (status, counters, f64 normals, f64 curvature, lists, NORMAL, Curvature)"""
        import torch
        n, k = self.n, self.k
        buf = self.strided if strided else self.packed
        buf.set_attribute_range(A.POSITION_3D, range(0, n), pts)
        pos, stride = self.source(strided)
        self.normals.view(torch.int64).fill_(-1)  # NaN bytes
        self.curv.view(torch.int64).fill_(-1)
        self.lists.fill_(-1)
        self.status.fill_(-1)
        torch.cuda.synchronize()
        assert self.hooks.replay(self.handle, pos, stride, self.status.data_ptr(), self.normals.data_ptr(), self.curv.data_ptr(), self.lists.data_ptr())
        torch.cuda.synchronize()
        c = self.hooks.counters(self.handle)
        st = [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.status.tolist()]
        assert st == status_restatement(c, self.facts), (st, c.n_finite, c.fb_count, c.box_count, list(c.open_count), c.error_count, self.facts.summary())
        assert st[1] == c.error_count
        hn, hc, hk = self.normals.cpu().numpy(), self.curv.cpu().numpy(), self.lists.cpu().numpy().view(np.uint32)
        public = []
        for t in (self.records, self.columns):
            t.reset()
            self.status.fill_(-1)
            torch.cuda.synchronize()
            self.public.compute_into_async(buf, t.buf, self.status.data_ptr())
            torch.cuda.synchronize()
            assert [int(v) & 0xFFFFFFFFFFFFFFFF for v in self.status.tolist()] == st, (t.kind, self.status.tolist(), st)
            pn, pc, intact = t.read()
            assert intact, f"{t.kind}: a guard band was written"
            public.append((pn, pc))
        if not st[0] & (BOX_CAPACITY | FALLBACK_CAPACITY):  # (beyond a capacity, WHICH boxes / hand-backs are served is decided by the order of atomics)
            assert public[0][0].tobytes() == public[1][0].tobytes() and public[0][1].tobytes() == public[1][1].tobytes(), "records and columns differ"
        return st, c, hn, hc, hk, public[0][0], public[0][1]

    def close(self):
        if self.public is not None:
            self.public.destroy()
            self.public = None
        if self.handle:
            self.hooks.plan_free(self.handle)
            self.handle = None


@contextlib.contextmanager
def _plan(hip, monkeypatch, pts, k, env=None, staged=False):
    p = _Plan(hip, monkeypatch, pts, k, env, staged)
    try:
        assert p.valid, p.why_not
        yield p
    finally:
        p.close()


def _assert_exact(plan, oracle, pts, result, ref, what):
    """what a replay without bits 0 - 3 owes: every row, against the oracle"""
    st, c, hn, hc, hk, pn, pc = result
    on, oc, ok = ref
    assert st == [0, 0], (what, st)
    assert np.array_equal(hk.astype(np.int64), ok), f"{what}: {int((hk.astype(np.int64) != ok).any(axis=1).sum())} neighbour lists differ from the oracle's"
    scales = gp._cov_scales(pts, ok)
    bad, cbad = gp._compare_normals(hn, hc, on, oc, scales=scales)
    rows = np.flatnonzero(bad | cbad)[:4]
    worst = [f"row {i}: normal {hn[i].tolist()} vs {on[i].tolist()}, curvature {float(hc[i])!r} vs {float(oc[i])!r}, scale {float(scales[i])!r}" for i in rows]
    assert pn.tobytes() == hn.astype(np.float32).tobytes(), f"{what}: the NORMAL column is not the narrowed f64 normal"
    assert pc.tobytes() == hc.tobytes(), f"{what}: the Curvature column differs from the f64 curvature"
    assert bad.sum() == 0 and cbad.sum() == 0, f"{what}: {int(bad.sum())} normals / {int(cbad.sum())} curvatures outside the window: {worst}"


def _assert_own_cloud(plan, result):
    """R0, the plan's own cloud: the columns of the synchronous call, bit for bit"""
    assert result[0] == [0, 0], result[0]
    assert result[5].tobytes() == plan.sync_want.view_attribute(A.NORMAL).tobytes() and result[6].tobytes() == plan.sync_want.view_attribute(CURV).tobytes()


def _same_rows(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))


_PLAN_ENV = {"V": {}, "S": {"PST_KNN_FORCE_TILE": "1"}, "T": {"PST_KNN_FORCE_TILE": "1"}}


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", _STATUS0, ids=[f"{p}-{w}" for p, w in _STATUS0])
def test_replay_status0_clouds_vs_oracle(hip, oracle, monkeypatch, name, which):
    """Plans V (a volume: every box launched, the one-pass fit), S (a surface under PST_KNN_FORCE_TILE: one workgroup per listed box, the
    reference-order fit) and T (a tilted slab: the rotated frame), k = 16, replayed on R0, on `which`, and on R0 again.  R3 - R5 and T31 put at
    least 1000 points outside the plan's box (asserted from the facts): clamped into boundary cells, searched exactly.  Status [0, 0] is owed
    in every case; no displacement had to be shrunk to stay inside fb_cap."""
    k = 16
    r0, pts = replay_cloud(name, "R0"), replay_cloud(name, which)
    with _plan(hip, monkeypatch, r0, k, _PLAN_ENV[name]) as plan:
        f = plan.facts
        print(name, which, f.summary())
        assert f.k == k and f.n == len(r0) and f.nf == len(r0)
        if name in _PLAN_H:
            assert f.h == pytest.approx(_PLAN_H[name], rel=1e-6), f"the recorded cell edge of plan {name} is stale: the device reports {f.h!r}"
        if name == "V":
            assert not f.use_list and not f.rotated and not f.staged
        if name == "S":
            assert f.use_list and f.fit_seq and f.list_cap >= f.n_list
        if name == "T":
            assert f.rotated
        assert plan.outside(r0) <= (1 if f.rotated else 0)  # (the host's rotated coordinates differ from the device's in the last bits)
        if which in ("R3", "R4", "R5", "T31"):
            assert plan.outside(pts) >= 1000, plan.outside(pts)
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        if which == "R0":
            _assert_exact(plan, oracle, r0, first, oracle_of(oracle, name, "R0", k), f"{name} R0")
        else:
            _assert_exact(plan, oracle, pts, plan.replay(pts), oracle_of(oracle, name, which, k), f"{name} {which}")
        again = plan.replay(r0)
        assert again[0] == [0, 0] and _same_rows(first, again)


@pytest.mark.gpu
@pytest.mark.parametrize("var", ["1", "B", "D", "G"])
@pytest.mark.parametrize("name,k", [("V", 8), ("V", 16), ("S", 8), ("S", 16)])
def test_replay_every_instance_of_the_box_kernel(hip, oracle, monkeypatch, name, k, var):
    """Every instance of the box kernel (PST_KNN_VAR at plan creation; the replay launches the instance its record names), on the volume
    and through the box list of the surface, k = 8 and 16: the plan's cloud and R5 (a layer of points beyond all six faces)."""
    r0, r5 = replay_cloud(name, "R0"), replay_cloud(name, "R5")
    with _plan(hip, monkeypatch, r0, k, dict(_PLAN_ENV[name], PST_KNN_VAR=var)) as plan:
        print(name, k, var, plan.facts.summary())
        assert plan.facts.tag == var and bool(plan.facts.use_list) == (name == "S")
        assert plan.outside(r5) >= 1000
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        _assert_exact(plan, oracle, r0, first, oracle_of(oracle, name, "R0", k), f"{name} k={k} {var} R0")
        _assert_exact(plan, oracle, r5, plan.replay(r5), oracle_of(oracle, name, "R5", k), f"{name} k={k} {var} R5")


@pytest.mark.gpu
@pytest.mark.parametrize("fit", ["seq", "pivot"])
def test_replay_both_fits(hip, oracle, monkeypatch, fit):
    """Plan V with the reference-order fit and with the one-pass fit (PST_KNN_FIT at plan creation): R0 and R5."""
    k = 16
    r0, r5 = replay_cloud("V", "R0"), replay_cloud("V", "R5")
    with _plan(hip, monkeypatch, r0, k, {"PST_KNN_FIT": fit}) as plan:
        assert bool(plan.facts.fit_seq) == (fit == "seq")
        assert plan.outside(r5) >= 1000
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        _assert_exact(plan, oracle, r0, first, oracle_of(oracle, "V", "R0", k), f"fit {fit} R0")
        _assert_exact(plan, oracle, r5, plan.replay(r5), oracle_of(oracle, "V", "R5", k), f"fit {fit} R5")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 9, 17, 24, 32, 33, 64])
def test_replay_other_list_lengths(hip, oracle, monkeypatch, k):
    """Plan V at list lengths on both sides of every instantiated K (8, 16, 32, 64), at the smallest and at the largest k: R0 and R5.
    (k = 33 and 64 take the box search -- the first form, tag '1' -- and so have a plan like the others: seen on the device, asserted here.)

    k = 3 found a defect of the one-pass fit: three points span a plane exactly, the determinant k0 of their covariance is rounding noise, and
    the reference's absolute test |k0| < 2.2e-16 for its quadratic branch (curvature 0) fell on the other side for the one-pass covariance
    of two nearly collinear triangles of R0 -- curvature 0.0 against the oracle's 1.90e-12 and 1.17e-12, windows 1.69e-12 and 1e-12, in the
    synchronous call and the replay alike.  Such a query now goes to the exact search, whose fit adds in the reference's order."""
    r0, r5 = replay_cloud("V", "R0"), replay_cloud("V", "R5")
    with _plan(hip, monkeypatch, r0, k) as plan:
        print(k, plan.facts.summary())
        assert plan.facts.k == k and plan.outside(r5) >= 1000
        if k > 16:
            assert plan.facts.tag == "1"
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        misses = []  # (both clouds are looked at before the case fails)
        for what, pts, result in (("R0", r0, first), ("R5", r5, plan.replay(r5))):
            try:
                _assert_exact(plan, oracle, pts, result, oracle_of(oracle, "V", what, k), f"k={k} {what}")
            except AssertionError as e:
                misses.append(str(e).splitlines()[0])
        assert not misses, misses


@pytest.mark.gpu
def test_replay_from_a_staged_source(hip, oracle, monkeypatch):
    """Plan V made on a VectorBuffer of [INTENSITY, POSITION_3D] packed (stride 26): the plans own a staging copy and replay from that buffer
    and from a HashMapBuffer alike (R0, then R4 with a slab of points beyond one face).  A plan made on a packed column has no staging copy
    and refuses the strided buffer on the host."""
    k = 16
    r0, r4 = replay_cloud("V", "R0"), replay_cloud("V", "R4")
    with _plan(hip, monkeypatch, r0, k, staged=True) as plan:
        assert plan.facts.staged and plan.source(True)[1] == 26
        assert plan.hooks.plan_accepts(plan.handle, *plan.source(True)) and plan.hooks.plan_accepts(plan.handle, *plan.source(False))
        assert plan.outside(r4) >= 1000
        first = plan.replay(r0, strided=True)
        _assert_own_cloud(plan, first)
        _assert_exact(plan, oracle, r0, first, oracle_of(oracle, "V", "R0", k), "staged R0")
        assert _same_rows(first, plan.replay(r0, strided=False))
        for strided in (True, False):
            _assert_exact(plan, oracle, r4, plan.replay(r4, strided=strided), oracle_of(oracle, "V", "R4", k), f"staged plan, strided source {strided}, R4")
        with _plan(hip, monkeypatch, r0, k) as packed_plan:
            assert not packed_plan.facts.staged
            assert not packed_plan.hooks.plan_accepts(packed_plan.handle, *plan.source(True))
            with pytest.raises(PastureError) as e:
                packed_plan.public.compute_into_async(plan.strided, plan.records.buf, plan.status.data_ptr())
            assert "the plan was made on a packed Vec3f64 position array" in e.value.message and "stride 26" in e.value.message


# ---- capacities and flags --------------------------------------------------------------------------------------------------------------------
def _assert_nothing_left_behind(plan, r0, first):
    """after a flagged replay: the plan's own cloud again -- status [0, 0], the rows of the first replay byte for byte"""
    again = plan.replay(r0)
    assert again[0] == [0, 0], again[0]
    assert _same_rows(first, again), "a flagged replay left something behind in the plan"


@pytest.mark.gpu
def test_replay_flags_an_exceeded_fallback_capacity(hip, monkeypatch):
    """Bit 2.  Plan V at 150 000 points, replayed on another seed scaled 3x about the centre: every query outside the box is handed back by
    the box kernel, and there are more of them than the hand-back list was sized for (counted on the host from the facts, before the replay)."""
    n, k = 150_000, 16
    r0, x3 = replay_cloud("V", "R0", n), replay_cloud("V", "X3", n)
    with _plan(hip, monkeypatch, r0, k) as plan:
        f = plan.facts
        print("V150", f.summary())
        outside = plan.outside(x3)
        assert outside > f.fb_cap, (outside, f.fb_cap)
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        st, c = plan.replay(x3)[:2]
        assert st[0] & FALLBACK_CAPACITY and c.fb_count >= outside and c.fb_count > f.fb_cap
        assert c.n_finite == n and not st[0] & FINITE_COUNT and not st[0] & BOX_CAPACITY
        assert bool(st[0] & OPEN_QUERIES) == bool(c.open_count[0] or c.open_count[1])
        _assert_nothing_left_behind(plan, r0, first)


def _two_sheets(seed, n, gap=600.0):
    """two copies of the surface generator, `gap` apart in z: a cloud whose grid is mostly empty boxes"""
    p = gp._planned_clouds(seed, n, "surface")
    p[n // 2:, 2] += gap
    return p


@pytest.mark.gpu
def test_replay_flags_an_exceeded_box_capacity(hip, monkeypatch):
    """Bit 1.  A list plan holds list_cap = min(all_boxes, n_list + n_list / 4 + 1024) boxes, so only a plan cloud that leaves most boxes of its
    grid empty can be overflowed.  Plan S never is such a cloud: its grid is one box deep in z and the surface fills every box -- the device
    reported n_list = list_cap = all_boxes = 144, 289, 441 and 868 at 100 000, 200 000, 300 000 and 600 000 points.  So this case plans two
    sheets of the same generator 600 apart in z at 200 000 points (under PST_KNN_FORCE_TILE: a list plan with empty layers of boxes between the
    sheets; the precondition list_cap < all_boxes is asserted from the facts), and replays a uniform cloud filling the plan's box, which
    occupies every box."""
    n, k = 200_000, 16
    r0 = _two_sheets(1, n)
    with _plan(hip, monkeypatch, r0, k, _PLAN_ENV["S"]) as plan:
        f = plan.facts
        print("two sheets", n, f.summary())
        assert f.use_list and f.list_cap < f.all_boxes, (f.n_list, f.list_cap, f.all_boxes)
        lo, hi = r0.min(axis=0), r0.max(axis=0)
        full = lo + np.random.default_rng(7).random((n, 3)) * (hi - lo)
        assert plan.outside(full) == 0
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        st, c = plan.replay(full)[:2]
        print("  uniform cloud in the box: status", st, "boxes", c.box_count, "fb", c.fb_count, "open", list(c.open_count))
        assert c.box_count > f.list_cap and st[0] & BOX_CAPACITY and not st[0] & FINITE_COUNT
        _assert_nothing_left_behind(plan, r0, first)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 65, N - 2])
def test_replay_flags_non_finite_points(hip, monkeypatch, m):
    """Bit 0: m non-finite points make the index shorter than planned.  Bit 4 and status2[1]: a fit is refused (Fit::ok == 0, counted by
    write_record) only for a neighbourhood of fewer than 3 points, m = min(nf, k) < 3 -- nf is the PLAN's count and k >= 3, the searches of a
    replay see finite points only, and a replay does not run the non-finite rows at all.  So NONE of the three sets bit 4: error_count stays
    0 (no replay of a valid plan can set it).  With two finite points left, both lack neighbours and stay open: bit 3."""
    k = 16
    r0 = replay_cloud("V", "R0")
    bad = r0.copy()
    rows = np.random.default_rng(3).choice(N, m, replace=False)
    bad[rows, np.arange(m) % 3] = np.array([np.nan, np.inf, -np.inf])[np.arange(m) % 3]
    with _plan(hip, monkeypatch, r0, k) as plan:
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        st, c = plan.replay(bad)[:2]
        assert st[0] & FINITE_COUNT and c.n_finite == N - m
        assert c.error_count == 0 and st[1] == 0 and not st[0] & DEGENERATE
        assert bool(st[0] & OPEN_QUERIES) == (m == N - 2)
        _assert_nothing_left_behind(plan, r0, first)


@pytest.mark.gpu
def test_replay_flags_open_queries_of_far_points(hip, monkeypatch):
    """Bit 3: three lone points 10^7 away are clamped into the plan's grid; the capped exact search hands their queries back."""
    k = 16
    r0 = replay_cloud("V", "R0")
    far = r0.copy()
    far[:3] += np.array([[1e7, 0, 0], [0, -2e7, 0], [0, 0, 3e7]])
    with _plan(hip, monkeypatch, r0, k) as plan:
        first = plan.replay(r0)
        _assert_own_cloud(plan, first)
        st, c = plan.replay(far)[:2]
        assert st == [OPEN_QUERIES, 0] and c.open_count[0] + c.open_count[1] >= 3
        _assert_nothing_left_behind(plan, r0, first)
