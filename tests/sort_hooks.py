"""ctypes binding of pasture_amd/csrc/build/libpst_sort_hooks.so (source: tests/cpp/sort_hooks.cpp): C forwarders to the sorts and scans of pasture_amd/csrc/device_sort.hpp
(pstk::radix_sort_pairs_u32 / _u64, sort_pairs_u32 / _u64, radix_sort_first_pass, radix_sort_pairs_supported, exclusive_sum_u32_u64,
suffix_min_u32).  Test infrastructure: built by `make -C pasture_amd/csrc`, i.e. by __graft_entry__.build(); not part of the C ABI.
Pointers are plain integers (torch's data_ptr(), 0 = nullptr); `bytes` is a ctypes.c_size_t passed by reference."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "pasture_amd", "csrc", "build", "libpst_sort_hooks.so")  # (build products stay out of tests/)

HIP_SUCCESS = 0
HIP_ERROR_INVALID_VALUE = 1

_P, _SZ, _U, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int
_PSZ = ctypes.POINTER(ctypes.c_size_t)

_SIGNATURES = {
    "sorthook_radix_sort_pairs_u32": (_I, [_P, _PSZ, _P, _P, _P, _P, _SZ, _U, _P, _I, _I]),
    "sorthook_radix_sort_pairs_u64": (_I, [_P, _PSZ, _P, _P, _P, _P, _SZ, _U, _P]),
    "sorthook_sort_pairs_u32": (_I, [_P, _PSZ, _P, _P, _P, _P, _SZ, _U, _P, _I]),
    "sorthook_sort_pairs_u64": (_I, [_P, _PSZ, _P, _P, _P, _P, _SZ, _U, _P]),
    "sorthook_radix_sort_first_pass": (None, [_P, _SZ, _U, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32)]),
    "sorthook_radix_sort_pairs_supported": (_I, [_SZ, _U]),
    "sorthook_exclusive_sum_u32_u64": (_I, [_P, _PSZ, _P, _P, _SZ, _P]),
    "sorthook_suffix_min_u32": (_I, [_P, _PSZ, _P, _SZ, _P]),
}


class SortHooks:
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
            setattr(self, "_" + name[len("sorthook_"):], fn)

    # every call returns the hipError_t as an int; `bytes_` is a ctypes.c_size_t the call may write (size query: tmp == 0)
    def radix_sort_pairs_u32(self, tmp, bytes_, keys_a, keys_b, vals_a, vals_b, n, end_bit, stream=0, iota=False, first_hist_ready=False):
        return self._radix_sort_pairs_u32(tmp, ctypes.byref(bytes_), keys_a, keys_b, vals_a, vals_b, n, end_bit, stream, int(iota), int(first_hist_ready))

    def radix_sort_pairs_u64(self, tmp, bytes_, keys_a, keys_b, vals_a, vals_b, n, end_bit, stream=0):
        return self._radix_sort_pairs_u64(tmp, ctypes.byref(bytes_), keys_a, keys_b, vals_a, vals_b, n, end_bit, stream)

    def sort_pairs_u32(self, tmp, bytes_, keys_in, keys_out, vals_in, vals_out, n, end_bit, stream=0, iota=False):
        return self._sort_pairs_u32(tmp, ctypes.byref(bytes_), keys_in, keys_out, vals_in, vals_out, n, end_bit, stream, int(iota))

    def sort_pairs_u64(self, tmp, bytes_, keys_in, keys_out, vals_in, vals_out, n, end_bit, stream=0):
        return self._sort_pairs_u64(tmp, ctypes.byref(bytes_), keys_in, keys_out, vals_in, vals_out, n, end_bit, stream)

    def radix_sort_first_pass(self, tmp, n, end_bit):
        """-> (counts address or 0, tiles, bits, tile_size): the four fields of RadixFirstPass"""
        counts, tiles, bits, tile_size = _P(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._radix_sort_first_pass(tmp, n, end_bit, ctypes.byref(counts), ctypes.byref(tiles), ctypes.byref(bits), ctypes.byref(tile_size))
        return counts.value or 0, tiles.value, bits.value, tile_size.value

    def radix_sort_pairs_supported(self, n, end_bit):
        return bool(self._radix_sort_pairs_supported(n, end_bit))

    def exclusive_sum_u32_u64(self, tmp, bytes_, in_, out, n, stream=0):
        return self._exclusive_sum_u32_u64(tmp, ctypes.byref(bytes_), in_, out, n, stream)

    def suffix_min_u32(self, tmp, bytes_, data, n, stream=0):
        return self._suffix_min_u32(tmp, ctypes.byref(bytes_), data, n, stream)


_hooks = None


def load():
    global _hooks
    if _hooks is None:
        _hooks = SortHooks()
    return _hooks
