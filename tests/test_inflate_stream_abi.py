"""The streaming-inflate part of the C ABI (include/mi355_deflate.h) without a GPU: the prototypes and the state record as C99, the
mirror's names and structures, the host build's item and record, and the argument errors, which are decided before a context or
the device is touched.  CPU only."""
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
    int (*mk)(mi355_deflate_ctx*, int, const uint8_t*, size_t, mi355_inflate_stream**) = 0;
    int (*wr)(mi355_inflate_stream*, const uint8_t*, size_t, uint8_t*, size_t, size_t*, mi355_inflate_report*) = 0;
    int (*wd)(mi355_inflate_stream*, const void*, size_t, void*, size_t, size_t*, mi355_inflate_report*, void*) = 0;
    int (*wb)(mi355_deflate_ctx*, mi355_inflate_stream* const*, mi355_batch_item*, size_t, mi355_inflate_report*, void*) = 0;
    int (*fin)(mi355_inflate_stream*, mi355_inflate_report*) = 0;
    int (*st)(mi355_inflate_stream*, mi355_inflate_stream_state*) = 0;
    int (*rs)(mi355_inflate_stream*) = 0;
    void (*fr)(mi355_inflate_stream*) = 0;
    int same = sizeof(mk == mi355_inflate_stream_new) + sizeof(wr == mi355_inflate_stream_write) + sizeof(wd == mi355_inflate_stream_write_device) +
               sizeof(wb == mi355_inflate_stream_write_batch_device) + sizeof(fin == mi355_inflate_stream_finish) +
               sizeof(st == mi355_inflate_stream_state_get) + sizeof(rs == mi355_inflate_stream_reset) + sizeof(fr == mi355_inflate_stream_free);
    printf("%d %d %d %d %d\n", (int)sizeof(mi355_inflate_stream_state), (int)offsetof(mi355_inflate_stream_state, need_out),
           (int)offsetof(mi355_inflate_stream_state, done), (int)offsetof(mi355_inflate_stream_state, adler_or_crc), same == 8 * (int)sizeof(int));
    return 0;
}
"""

NAMES = ("mi355_inflate_stream_new", "mi355_inflate_stream_write", "mi355_inflate_stream_write_device",
         "mi355_inflate_stream_write_batch_device", "mi355_inflate_stream_finish", "mi355_inflate_stream_state_get",
         "mi355_inflate_stream_reset", "mi355_inflate_stream_free")


def test_the_header_is_c99_and_names_the_entry_points(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    S = da.InflateStreamState
    assert got == [C.sizeof(S), S.need_out.offset, S.done.offset, S.adler_or_crc.offset, 1]
    assert got[0] == 48


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in NAMES:
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("inflate_stream", "inflate_stream_write_batch", "inflate_stream_write_batch_device"):
        assert callable(getattr(da.Context, name))
    for name in ("write", "write_raw", "write_device", "finish", "finish_raw", "state", "reset", "close"):
        assert callable(getattr(da.InflateStream, name))
    assert isinstance(da.InflateStream.done, property)


def test_the_host_builds_state_is_the_abis():
    import inflstream_binding as sb
    assert C.sizeof(sb.State) == 48
    assert [f for f, _ in sb.State._fields_] == ["total_in", "total_out", "pending_in", "need_out", "done", "failed", "adler_or_crc", "reserved"]


def test_argument_errors_come_before_the_device():
    """ctx NULL: were the device touched, a machine without one would answer MI355_E_HIP"""
    import deflate_amd as da
    L = da.load()
    r = da.InflateReport()
    n = C.c_size_t(0)
    h = C.c_void_p()
    st = da.InflateStreamState()
    E_ARG = da.E_ARG
    assert L.mi355_inflate_stream_new(None, 3, None, 0, C.byref(h)) == E_ARG
    assert L.mi355_inflate_stream_new(None, -1, None, 0, C.byref(h)) == E_ARG
    assert L.mi355_inflate_stream_new(None, 0, None, 0, None) == E_ARG
    assert L.mi355_inflate_stream_new(None, 0, None, 5, C.byref(h)) == E_ARG       # a length without a dictionary
    assert L.mi355_inflate_stream_new(None, 1, b"dict", 4, C.byref(h)) == E_ARG    # a dictionary goes with a raw stream only
    assert L.mi355_inflate_stream_new(None, 2, b"dict", 4, C.byref(h)) == E_ARG
    assert not h.value
    assert L.mi355_inflate_stream_write(None, b"x", 1, None, 0, C.byref(n), C.byref(r)) == E_ARG
    assert L.mi355_inflate_stream_write_device(None, None, 0, None, 0, C.byref(n), C.byref(r), None) == E_ARG
    assert L.mi355_inflate_stream_finish(None, C.byref(r)) == E_ARG
    assert L.mi355_inflate_stream_state_get(None, C.byref(st)) == E_ARG
    assert L.mi355_inflate_stream_reset(None) == E_ARG
    L.mi355_inflate_stream_free(None)
    # with a handle in hand the other pointers are looked at first: a handle that is no handle is never dereferenced
    fake = C.c_void_p(8)
    buf = C.create_string_buffer(16)
    assert L.mi355_inflate_stream_write(fake, b"x", 1, buf, 16, None, C.byref(r)) == E_ARG
    assert L.mi355_inflate_stream_write(fake, b"x", 1, buf, 16, C.byref(n), None) == E_ARG
    assert L.mi355_inflate_stream_write(fake, None, 1, buf, 16, C.byref(n), C.byref(r)) == E_ARG
    assert L.mi355_inflate_stream_write(fake, b"x", 1, None, 16, C.byref(n), C.byref(r)) == E_ARG
    assert L.mi355_inflate_stream_write_device(fake, None, 1, None, 0, C.byref(n), C.byref(r), None) == E_ARG
    assert L.mi355_inflate_stream_finish(fake, None) == E_ARG
    assert L.mi355_inflate_stream_state_get(fake, None) == E_ARG
    # the batch: NULL arrays, a NULL handle, an item without buffers, the same handle twice
    items = (da.BatchItem * 2)()
    hs = (C.c_void_p * 2)(None, None)
    assert L.mi355_inflate_stream_write_batch_device(None, None, items, 2, None, None) == E_ARG
    assert L.mi355_inflate_stream_write_batch_device(None, hs, None, 2, None, None) == E_ARG
    assert L.mi355_inflate_stream_write_batch_device(None, hs, items, 2, None, None) == E_ARG
    hs = (C.c_void_p * 2)(8, 16)
    items[0].in_len = 4
    assert L.mi355_inflate_stream_write_batch_device(None, hs, items, 2, None, None) == E_ARG
    items[0].in_len, items[1].out_cap = 0, 4
    assert L.mi355_inflate_stream_write_batch_device(None, hs, items, 2, None, None) == E_ARG
    items[1].out_cap = 0
    hs = (C.c_void_p * 2)(8, 8)
    assert L.mi355_inflate_stream_write_batch_device(None, hs, items, 2, None, None) == E_ARG
