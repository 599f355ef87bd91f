"""The test build of the library (deflate-rs_amd/libmi355deflate_dbg.so: `make debug`, -DMI355_DEBUG_HOOKS) through ctypes, for the
GPU tests that read the sort's tables or force its mark (tests/test_sort_gpu.py, tests/test_match_walk_swz_gpu.py).  The test
build is a compile of its own: the same source with one dead branch more in k_sort (the hooks' bits of its `dbl` argument), so
what a test sees through a hook is also run on the product library for its bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deflate-rs_amd")
sys.path.insert(0, PKG)

EPOCH = 32768
BSTRIDE = EPOCH + 8
_lib = None


def load():
    """the library, built first if it is missing (as tests/test_gpu_parity.py test_sort_order_is_checked_on_the_data does)"""
    global _lib
    if _lib is not None:
        return _lib
    import deflate_amd as da
    path = os.path.join(PKG, "libmi355deflate_dbg.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", PKG, "-s", "debug"])
    L = C.CDLL(path)
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    L.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mi355_deflate_ctx_destroy.argtypes = [C.c_void_p]
    L.mi355_deflate_ctx_destroy.restype = None
    L.mi355_deflate_last_error.argtypes = [C.c_void_p]
    L.mi355_deflate_last_error.restype = C.c_char_p
    L.mi355_deflate_bound.argtypes = [C.c_size_t]
    L.mi355_deflate_bound.restype = C.c_size_t
    L.mi355_deflate_bound_ex.argtypes = [C.c_size_t, C.c_int, C.c_size_t, C.c_size_t]
    L.mi355_deflate_bound_ex.restype = C.c_size_t
    L.mi355_deflate_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(da.Opts), u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_deflate_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(da.Opts), C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_size_t), C.c_void_p]
    L.mi355_deflate_encode_batch.argtypes = [C.c_void_p, C.POINTER(da.BatchItem), C.c_size_t, C.POINTER(da.Opts)]
    L.mi355_deflate_last_info.argtypes = [C.c_void_p, C.POINTER(da.Info)]
    L.mi355_deflate_last_blocks.argtypes = [C.c_void_p, C.POINTER(da.BlockInfo), C.c_size_t, C.POINTER(C.c_size_t)]
    L.mi355_deflate_ctx_config.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.mi355_debug_break_sort.argtypes = [C.c_void_p, C.c_int]
    L.mi355_debug_sort_ranks.argtypes = [C.c_void_p]
    L.mi355_debug_sort_tables.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, u16p, u16p]
    L.mi355_debug_force_swz.argtypes = [C.c_void_p, C.c_int]
    _lib = L
    return L


class Ctx:
    """a context of the test build"""

    def __init__(self, device=0):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.mi355_deflate_ctx_create(device, C.byref(self.h))
        assert rc == 0, "no context on the test build (%d)" % rc

    def close(self):
        if self.h:
            self.L.mi355_deflate_ctx_destroy(self.h)
            self.h = None

    def _ok(self, rc, what):
        assert rc == 0, "%s: %d (%s)" % (what, rc, self.L.mi355_deflate_last_error(self.h).decode())

    def config(self, key, value):
        self._ok(self.L.mi355_deflate_ctx_config(self.h, int(key), int(value)), "config")

    def sort_ranks(self):
        return self.L.mi355_debug_sort_ranks(self.h)

    def force_swz(self, mode):
        self._ok(self.L.mi355_debug_force_swz(self.h, mode), "mi355_debug_force_swz")

    def encode(self, data, opts, compat=1):
        import deflate_amd as da
        o = da.CompressionOptions(*opts).to_c(0, compat, 0)
        cap = self.L.mi355_deflate_bound(len(data)) + 16
        out = (C.c_uint8 * cap)()
        n = C.c_size_t(0)
        self._ok(self.L.mi355_deflate_encode(self.h, bytes(data), len(data), C.byref(o), out, cap, C.byref(n)), "encode")
        return bytes(memoryview(out)[:n.value])

    def encode_device(self, d_in, n_in, d_out, cap, opts, compat=1):
        import deflate_amd as da
        o = da.CompressionOptions(*opts).to_c(0, compat, 0)
        n = C.c_size_t(0)
        self._ok(self.L.mi355_deflate_encode_device(self.h, C.c_void_p(d_in), n_in, C.byref(o), C.c_void_p(d_out), cap, C.byref(n), None),
                 "encode_device")
        return n.value

    def encode_batch(self, datas, opts, compat=1):
        import deflate_amd as da
        o = da.CompressionOptions(*opts).to_c(0, compat, 0)
        datas = [bytes(d) for d in datas]
        items = (da.BatchItem * max(len(datas), 1))()
        outs = []
        for k, d in enumerate(datas):
            cap = self.L.mi355_deflate_bound_ex(len(d), 0, 0, 0)
            out = (C.c_uint8 * max(cap, 1))()
            outs.append(out)
            items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
            items[k].in_len = len(d)
            items[k].out = C.cast(out, C.c_void_p)
            items[k].out_cap = cap
        self._ok(self.L.mi355_deflate_encode_batch(self.h, items, len(datas), C.byref(o)), "encode_batch")
        return [bytes(memoryview(outs[k])[:items[k].out_len]) for k in range(len(datas))]

    def passes(self):
        import deflate_amd as da
        i = da.Info()
        self.L.mi355_deflate_last_info(self.h, C.byref(i))
        return i.passes

    def blocks(self):
        import deflate_amd as da
        n = C.c_size_t(0)
        self.L.mi355_deflate_last_blocks(self.h, None, 0, C.byref(n))
        arr = (da.BlockInfo * max(n.value, 1))()
        self._ok(self.L.mi355_deflate_last_blocks(self.h, arr, n.value, C.byref(n)), "last_blocks")
        return [dict(btype=a.btype, bfinal=a.bfinal, n_lz=a.n_tokens, in_bytes=a.in_bytes, bit_start=a.bit_start) for a in arr[:n.value]]

    def tables(self, ne, e0=0):
        """(S, B) of epochs e0 .. e0 + ne - 1 of the last single-pass call: uint16 arrays [ne, 32768] and [ne, BSTRIDE]"""
        S = np.zeros((max(ne, 1), EPOCH), dtype=np.uint16)
        B = np.zeros((max(ne, 1), BSTRIDE), dtype=np.uint16)
        rc = self.L.mi355_debug_sort_tables(self.h, e0, ne, S.ctypes.data_as(C.POINTER(C.c_uint16)), B.ctypes.data_as(C.POINTER(C.c_uint16)))
        self._ok(rc, "mi355_debug_sort_tables(%d, %d)" % (e0, ne))
        return S[:ne], B[:ne]

    def tables_rc(self, ne, e0=0):
        S = np.zeros((max(ne, 1), EPOCH), dtype=np.uint16)
        B = np.zeros((max(ne, 1), BSTRIDE), dtype=np.uint16)
        return self.L.mi355_debug_sort_tables(self.h, e0, ne, S.ctypes.data_as(C.POINTER(C.c_uint16)), B.ctypes.data_as(C.POINTER(C.c_uint16)))
