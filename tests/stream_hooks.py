"""ctypes binding of pasture_amd/csrc/build/libpst_stream_hooks.so (source: tests/cpp/stream_hooks.cpp): C forwarders to the fused Vec3f64 stream
and the AABB record fold of pasture_amd/csrc/stream.hip (pstk::stream_partials_bytes, launch_vec3f64_stream, bounds_partials_bytes,
launch_finalize_bounds, set_bounds_record_form).
Test infrastructure: built by `make -C pasture_amd/csrc`, i.e. by __graft_entry__.build(); not part of the C ABI.
Pointers are plain integers (torch's data_ptr(), 0 = nullptr)."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "pasture_amd", "csrc", "build", "libpst_stream_hooks.so")  # (build products stay out of tests/)

_P, _SZ, _U32, _U64, _INT = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
_D3 = ctypes.c_double * 3

_SIGNATURES = {
    "streamhook_partials_bytes": (_SZ, [_U64, _U32]),
    "streamhook_launch": (None, [_P, _P, _U64, ctypes.POINTER(_D3), ctypes.POINTER(_D3), _U32, _P, _P, _P]),
    "streamhook_bounds_partials_bytes": (_SZ, [_U32]),
    "streamhook_finalize_bounds": (None, [_P, _U32, _P, _P, _U64, _U64, _U64]),
    "streamhook_set_record_form": (None, [_P, _INT]),
}


class StreamHooks:
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
            setattr(self, "_" + name[len("streamhook_"):], fn)

    def partials_bytes(self, n_points, mode):
        return int(self._partials_bytes(n_points, mode))

    def launch(self, src, dst, n_points, scale, offset, mode, partials, out6, stream=0):
        """scale / offset: three floats each, or None (identity)"""
        s = None if scale is None else ctypes.byref(_D3(*[float(x) for x in scale]))
        o = None if offset is None else ctypes.byref(_D3(*[float(x) for x in offset]))
        self._launch(src, dst, n_points, s, o, mode, partials, out6, stream)

    def bounds_partials_bytes(self, n_records):
        return int(self._bounds_partials_bytes(n_records))

    def finalize_bounds(self, partials, n_records, out6, stream=0, zero_base=0, zero_stride=0, zero_n=0):
        self._finalize_bounds(partials, n_records, out6, stream, zero_base, zero_stride, zero_n)

    def set_record_form(self, rec, form):
        self._set_record_form(rec, form)


_hooks = None


def load():
    global _hooks
    if _hooks is None:
        _hooks = StreamHooks()
    return _hooks
