"""The index part of the C ABI (include/mi355_deflate.h) without a GPU: the prototypes, the record and the new setting as C99, the
mirror's names, the host build's record, and the argument errors of an index or a parallel call, which are decided before a context
or the device is touched.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "mi355_deflate.h"
int main(void) {
    /* the prototypes, compared inside sizeof: checked by the compiler, nothing to link */
    int (*xdev)(mi355_deflate_ctx*, const void*, size_t, int, mi355_block_info*, size_t, size_t*, mi355_inflate_report*, void*) = 0;
    int (*xhost)(mi355_deflate_ctx*, const uint8_t*, size_t, int, mi355_block_info*, size_t, size_t*, mi355_inflate_report*) = 0;
    int (*pdev)(mi355_deflate_ctx*, const void*, size_t, int, void*, size_t, size_t*, mi355_inflate_report*, void*) = 0;
    int (*phost)(mi355_deflate_ctx*, const uint8_t*, size_t, int, uint8_t*, size_t, size_t*, mi355_inflate_report*) = 0;
    int (*stages)(mi355_deflate_ctx*, float*) = 0;
    int (*walks)(mi355_deflate_ctx*, mi355_index_walk*, size_t, size_t*) = 0;
    int same = sizeof(xdev == mi355_inflate_index_device) + sizeof(xhost == mi355_inflate_index) +
               sizeof(pdev == mi355_inflate_parallel_device) + sizeof(phost == mi355_inflate_parallel) +
               sizeof(stages == mi355_inflate_index_last_stages) + sizeof(walks == mi355_inflate_index_last_walks);
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(mi355_inflate_report), (int)sizeof(mi355_block_info), (int)sizeof(mi355_index_walk),
           (int)offsetof(mi355_index_walk, how), (int)offsetof(mi355_index_walk, n_blocks), MI355_CFG_INFLATE_INDEX_SPAN_BYTES,
           same == 6 * (int)sizeof(int));
    return 0;
}
"""

NAMES = ("mi355_inflate_index", "mi355_inflate_index_device", "mi355_inflate_parallel", "mi355_inflate_parallel_device",
         "mi355_inflate_index_last_stages", "mi355_inflate_index_last_walks")


def test_the_header_is_c99_and_names_the_entry_points_and_the_setting(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    W = da.IndexWalk
    assert got == [C.sizeof(da.InflateReport), C.sizeof(da.BlockInfo), C.sizeof(W), W.how.offset, W.n_blocks.offset,
                   da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, 1]
    assert got[:3] == [56, 32, 80] and got[5] == 12


def test_the_mirror_names_the_entry_points():
    import inspect

    import deflate_amd as da
    for name in NAMES:
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for fn in (da.Context.inflate, da.Context.inflate_raw, da.Context.inflate_device, da.inflate_bytes):
        assert inspect.signature(fn).parameters["parallel"].default is False
    for name in ("inflate_index", "inflate_index_device", "inflate_index_stages"):
        assert callable(getattr(da.Context, name))


def test_the_host_builds_record_is_the_abis():
    import deflate_amd as da
    import inflindex_binding as xb
    L = xb.lib()
    assert L.inflindex_walk_size() == C.sizeof(da.IndexWalk) == C.sizeof(xb.Walk) == 80
    assert [f for f, _t in xb.Walk._fields_] == [f for f, _t in da.IndexWalk._fields_]
    assert C.sizeof(xb.BlockInfo) == C.sizeof(da.BlockInfo) and [f for f, _t in xb.BlockInfo._fields_] == [f for f, _t in da.BlockInfo._fields_]
    assert L.inflindex_span_min() == 256
    assert xb.STATUS == da.VERIFY_STATUS and (xb.E_DATA, xb.E_OUT_TOO_SMALL, xb.E_ARG) == (da.E_DATA, da.E_OUT_TOO_SMALL, da.E_ARG)


def test_argument_errors_come_before_the_device():
    """ctx NULL: were the device touched, a machine without one would answer MI355_E_HIP"""
    import deflate_amd as da
    L = da.load()
    n, r = C.c_size_t(0), da.InflateReport()
    s = C.create_string_buffer(b"\x03\x00", 2)
    sp = C.cast(s, C.c_void_p)
    out = C.create_string_buffer(16)
    op = C.cast(out, C.c_void_p)
    blocks = (da.BlockInfo * 4)()
    for fn, sarg in ((L.mi355_inflate_index_device, sp), (L.mi355_inflate_index, s.raw)):
        tail = (None,) if fn is L.mi355_inflate_index_device else ()
        assert fn(None, sarg, 2, 3, blocks, 4, C.byref(n), C.byref(r), *tail) == da.E_ARG   # wrapper
        assert fn(None, sarg, 2, -1, blocks, 4, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, None, 2, 0, blocks, 4, C.byref(n), C.byref(r), *tail) == da.E_ARG   # a length without a stream
        assert fn(None, sarg, 2, 0, None, 4, C.byref(n), C.byref(r), *tail) == da.E_ARG     # room without a table
        assert fn(None, sarg, 2, 0, blocks, 4, None, C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, blocks, 4, C.byref(n), None, *tail) == da.E_ARG
    for fn, sarg in ((L.mi355_inflate_parallel_device, sp), (L.mi355_inflate_parallel, s.raw)):
        tail = (None,) if fn is L.mi355_inflate_parallel_device else ()
        assert fn(None, sarg, 2, 3, op, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, -1, op, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, None, 2, 0, op, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, None, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG    # a size without a buffer
        assert fn(None, sarg, 2, 0, op, 16, None, C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, op, 16, C.byref(n), None, *tail) == da.E_ARG
    # the span size: 256 bytes at least, 1 GiB at most
    for bad in (0, 255, (1 << 30) + 1):
        assert L.mi355_deflate_ctx_config(None, da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, bad) == da.E_ARG
    ms = (C.c_float * 3)()
    assert L.mi355_inflate_index_last_stages(None, ms) == da.E_ARG
    assert L.mi355_inflate_index_last_walks(None, None, 0, C.byref(n)) == da.E_ARG


def test_parallel_together_with_blocks_is_an_error():
    """decided in the mirror, before the library is asked for a context"""
    import pytest

    import deflate_amd as da
    c = da.Context.__new__(da.Context)  # (no device: the methods below must refuse before they use the handle)
    c._h = None
    for call in (lambda: c.inflate_raw(b"\x03\x00", 0, 16, blocks=[(0, 0)], parallel=True),
                 lambda: c.inflate(b"\x03\x00", 0, 16, blocks=[(0, 0)], parallel=True),
                 lambda: c.inflate_device(0, 2, 0, 0, blocks=[(0, 0)], parallel=True)):
        with pytest.raises(ValueError):
            call()
