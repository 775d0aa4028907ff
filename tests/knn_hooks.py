"""ctypes binding of pasture_amd/csrc/build/libpst_knn_hooks.so (source: tests/cpp/knn_hooks.cpp): C forwarders to the stream-ordered replay of
compute_normals in pasture_amd/csrc/normals.hip (pstk::run_normals with a record, knn_plan_create / knn_plan_free, run_normals_replay with all
three device outputs or attribute targets) and read-only views of a plan (its record, its capacities, the counters of its latest replay).
Test infrastructure: built by `make -C pasture_amd/csrc`, i.e. by __graft_entry__.build(); not part of the C ABI.
Pointers are plain integers (torch's data_ptr(), 0 = nullptr)."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "pasture_amd", "csrc", "build", "libpst_knn_hooks.so")  # (build products stay out of tests/)

_P, _I, _U32, _U64, _LL, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_double


class KnnFacts(ctypes.Structure):
    """knnhook_facts, field for field"""
    _fields_ = [("n", _U64), ("nf", _U64), ("cells", _U64),
                ("org", _D * 3), ("h", _D), ("rot", _D * 9), ("rot_c", _D * 3),
                ("dim", _U32 * 3), ("rx", _U32), ("rotated", _U32),
                ("k", _U32), ("key_bits", _U32),
                ("bx", _U32), ("by", _U32), ("bz", _U32), ("threads", _U32), ("cap", _U32), ("tag_code", _U32), ("fit_seq", _U32),
                ("use_list", _U32), ("n_list", _U32), ("n_fb", _U32), ("all_boxes", _U32), ("list_cap", _U32), ("fb_cap", _U32), ("staged", _U32)]

    @property
    def tag(self):
        return chr(self.tag_code)

    def summary(self):
        return {f: getattr(self, f) for f in ("n_fb", "fb_cap", "n_list", "list_cap", "all_boxes", "tag", "use_list", "fit_seq", "rotated", "h", "rx", "staged")}


class KnnCounters(ctypes.Structure):
    """knnhook_counters, field for field"""
    _fields_ = [("n_finite", _U64), ("fb_count", _U32), ("box_count", _U32), ("open_count", _U32 * 2), ("error_count", ctypes.c_int32)]


_SIGNATURES = {
    "knnhook_run_normals": (_LL, [_P, _U64, _U64, _U32, _P, _P, _P, _U64, _U64, _U64, _U64, _P, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_char_p)]),
    "knnhook_record_free": (None, [_P]),
    "knnhook_plan_create": (_P, [_P, _I, _P]),
    "knnhook_plan_free": (None, [_P]),
    "knnhook_plan_accepts": (_I, [_P, _P, _U64]),
    "knnhook_replay": (_I, [_P, _P, _U64, _P, _P, _P, _U64, _U64, _U64, _U64, _P, _P]),
    "knnhook_plan_facts": (None, [_P, ctypes.POINTER(KnnFacts)]),
    "knnhook_plan_counters": (_I, [_P, ctypes.POINTER(KnnCounters), _P]),
}


class KnnHooks:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run build() of __graft_entry__.py (make -C pasture_amd/csrc)")
        # one process holds ONE HIP runtime (pasture_amd/_capi.py): torch's has to be the first one loaded, or the kernels launched through
        # this library would go to a second runtime that knows none of torch's allocations and streams
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
            setattr(self, "_" + name[len("knnhook_"):], fn)

    def run_normals(self, pos, stride, n, k, normals=0, curvature=0, knn=0, normal_attr=0, normal_stride=0, curv_attr=0, curv_stride=0, stream=0):
        """pstk::run_normals with a record -> (return code, record handle, valid, why_not); the handle goes to record_free"""
        rec, valid, why = _P(), _I(), ctypes.c_char_p()
        rc = self._run_normals(pos, stride, n, k, normals, curvature, knn, normal_attr, normal_stride, curv_attr, curv_stride, stream, ctypes.byref(rec), ctypes.byref(valid),
                               ctypes.byref(why))
        return int(rc), rec.value, bool(valid.value), (why.value or b"").decode()

    def record_free(self, record):
        self._record_free(record)

    def plan_create(self, record, packed_source, stream=0):
        return self._plan_create(record, 1 if packed_source else 0, stream) or 0

    def plan_free(self, plan):
        self._plan_free(plan)

    def plan_accepts(self, plan, pos, stride):
        return bool(self._plan_accepts(plan, pos, stride))

    def replay(self, plan, pos, stride, status2, normals=0, curvature=0, knn=0, normal_attr=0, normal_stride=0, curv_attr=0, curv_stride=0, stream=0):
        """pstk::run_normals_replay (launches only; the caller synchronises) -> False on a HIP failure"""
        return bool(self._replay(plan, pos, stride, normals, curvature, knn, normal_attr, normal_stride, curv_attr, curv_stride, status2, stream))

    def facts(self, plan):
        f = KnnFacts()
        self._plan_facts(plan, ctypes.byref(f))
        return f

    def counters(self, plan, stream=0):
        """the plan's device counters after its latest replay (synchronises the stream)"""
        c = KnnCounters()
        if not self._plan_counters(plan, ctypes.byref(c), stream):
            raise RuntimeError("knnhook_plan_counters: the copy failed")
        return c


_hooks = None


def load():
    global _hooks
    if _hooks is None:
        _hooks = KnnHooks()
    return _hooks
