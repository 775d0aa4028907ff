"""ctypes binding of pasture_amd/csrc/build/libpst_filter_hooks.so (source: tests/cpp/filter_hooks.cpp): C forwarders to the count and scan
phase of the compaction in pasture_amd/csrc/filter.hip (pstk::filter_workspace_bytes, filter_tile, launch_filter_count, filter_counts).
Test infrastructure: built by `make -C pasture_amd/csrc`, i.e. by __graft_entry__.build(); not part of the C ABI.
Pointers are plain integers (torch's data_ptr(), 0 = nullptr)."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "pasture_amd", "csrc", "build", "libpst_filter_hooks.so")  # (build products stay out of tests/)

_P, _SZ, _U32, _U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64

_SIGNATURES = {
    "filterhook_workspace_bytes": (_SZ, [_U64]),
    "filterhook_tile": (_U32, []),
    "filterhook_count": (_P, [_P, _U64, _U32, _P, _P, _P]),
    "filterhook_layout": (None, [_P, _U64, _U32, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
}


class FilterHooks:
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
            setattr(self, "_" + name[len("filterhook_"):], fn)

    def workspace_bytes(self, n):
        return int(self._workspace_bytes(n))

    def tile(self):
        return int(self._tile())

    def count(self, mask, n, tile, workspace, stream=0, total_also=0):
        """counts and offsets of `mask` into `workspace`, on `stream`; -> the address the launch names for the total"""
        return self._count(mask, n, tile, workspace, stream, total_also) or 0

    def layout(self, workspace, n, tile):
        """-> (offsets address, counts address) inside the workspace"""
        offsets, counts = _P(), _P()
        self._layout(workspace, n, tile, ctypes.byref(offsets), ctypes.byref(counts))
        return offsets.value or 0, counts.value or 0


_hooks = None


def load():
    global _hooks
    if _hooks is None:
        _hooks = FilterHooks()
    return _hooks
