"""The seek part of the C ABI (include/mi355_deflate.h) without a GPU: the prototypes and the records as C99, the mirror's names and
structures, the host build's descriptor, and the argument errors of a build and of a read, which are decided before a context or the
device is touched.  CPU only."""
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
    int (*bdev)(mi355_deflate_ctx*, const void*, size_t, int, const mi355_block_info*, size_t, uint64_t, mi355_inflate_seek**,
                mi355_inflate_report*, void*) = 0;
    int (*bhost)(mi355_deflate_ctx*, const uint8_t*, size_t, int, const mi355_block_info*, size_t, uint64_t, mi355_inflate_seek**,
                 mi355_inflate_report*) = 0;
    void (*fr)(mi355_inflate_seek*) = 0;
    int (*info)(mi355_inflate_seek*, mi355_seek_info*) = 0;
    int (*points)(mi355_inflate_seek*, mi355_seek_point*, size_t, size_t*) = 0;
    int (*rdev)(mi355_inflate_seek*, const void*, uint64_t, uint64_t, void*, uint64_t*, mi355_inflate_report*, void*) = 0;
    int (*rhost)(mi355_inflate_seek*, uint64_t, uint64_t, uint8_t*, uint64_t*, mi355_inflate_report*) = 0;
    int (*rbatch)(mi355_inflate_seek*, const void*, mi355_seek_range*, size_t, mi355_inflate_report*, void*) = 0;
    int (*last)(mi355_inflate_seek*, uint64_t*) = 0;
    int same = sizeof(bdev == mi355_inflate_seek_build_device) + sizeof(bhost == mi355_inflate_seek_build) +
               sizeof(fr == mi355_inflate_seek_free) + sizeof(info == mi355_inflate_seek_info) + sizeof(points == mi355_inflate_seek_points) +
               sizeof(rdev == mi355_inflate_seek_read_device) + sizeof(rhost == mi355_inflate_seek_read) +
               sizeof(rbatch == mi355_inflate_seek_read_batch_device) + sizeof(last == mi355_inflate_seek_last_read);
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(mi355_seek_info), (int)sizeof(mi355_seek_point), (int)sizeof(mi355_seek_range),
           (int)offsetof(mi355_seek_info, wrapper), (int)offsetof(mi355_seek_range, got), (int)offsetof(mi355_seek_range, status),
           same == 9 * (int)sizeof(int));
    return 0;
}
"""

NAMES = ("mi355_inflate_seek_build", "mi355_inflate_seek_build_device", "mi355_inflate_seek_free", "mi355_inflate_seek_info",
         "mi355_inflate_seek_points", "mi355_inflate_seek_read", "mi355_inflate_seek_read_device", "mi355_inflate_seek_read_batch_device",
         "mi355_inflate_seek_last_read")


def test_the_header_is_c99_and_names_the_entry_points(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    assert got == [C.sizeof(da.SeekInfo), C.sizeof(da.SeekPoint), C.sizeof(da.SeekRange), da.SeekInfo.wrapper.offset, da.SeekRange.got.offset,
                   da.SeekRange.status.offset, 1]
    assert got[:3] == [56, 16, 40]


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in NAMES:
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("inflate_seek", "inflate_seek_device"):
        assert callable(getattr(da.Context, name))
    for name in ("read", "read_raw", "read_batch", "read_device", "read_batch_device", "info", "points", "last_read", "close"):
        assert callable(getattr(da.SeekIndex, name))


def test_the_host_builds_descriptor_is_the_kernels():
    import inflseek_binding as sb
    assert sb.lib().inflseek_part_size() == 88


def test_argument_errors_come_before_the_device():
    """ctx NULL: were the device touched, a machine without one would answer MI355_E_HIP"""
    import deflate_amd as da
    L = da.load()
    r = da.InflateReport()
    h = C.c_void_p()
    s = C.create_string_buffer(b"\x03\x00", 2)
    sp = C.cast(s, C.c_void_p)
    good = (da.BlockInfo * 1)()
    late = (da.BlockInfo * 1)()
    late[0].bit_start = 3
    down = (da.BlockInfo * 2)()
    down[0].bit_start, down[1].bit_start = 8, 0
    for fn, sarg in ((L.mi355_inflate_seek_build_device, sp), (L.mi355_inflate_seek_build, s.raw)):
        tail = (None,) if fn is L.mi355_inflate_seek_build_device else ()
        assert fn(None, None, 2, 0, None, 0, 0, C.byref(h), C.byref(r), *tail) == da.E_ARG        # a length without a stream
        assert fn(None, sarg, 2, 3, None, 0, 0, C.byref(h), C.byref(r), *tail) == da.E_ARG        # wrapper
        assert fn(None, sarg, 2, -1, None, 0, 0, C.byref(h), C.byref(r), *tail) == da.E_ARG
        for spacing in (1, 32767, (1 << 30) + 1, 1 << 31):
            assert fn(None, sarg, 2, 0, None, 0, spacing, C.byref(h), C.byref(r), *tail) == da.E_ARG
            assert fn(None, sarg, 2, 0, good, 1, spacing, C.byref(h), C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, late, 1, 0, C.byref(h), C.byref(r), *tail) == da.E_ARG        # a table not from bit 0
        assert fn(None, sarg, 2, 0, down, 2, 0, C.byref(h), C.byref(r), *tail) == da.E_ARG        # ... whose bits descend
        assert fn(None, sarg, 2, 0, None, 0, 0, None, C.byref(r), *tail) == da.E_ARG              # nowhere to leave the handle
        assert fn(None, sarg, 2, 0, None, 0, 0, C.byref(h), None, *tail) == da.E_ARG
        assert h.value is None
    # reads: a NULL handle, a NULL got
    got = C.c_uint64(0)
    out = C.create_string_buffer(16)
    op = C.cast(out, C.c_void_p)
    assert L.mi355_inflate_seek_read_device(None, sp, 0, 16, op, C.byref(got), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_seek_read_device(None, sp, 0, 16, op, None, C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_seek_read(None, 0, 16, op, C.byref(got), C.byref(r)) == da.E_ARG
    assert L.mi355_inflate_seek_read(None, 0, 16, op, None, C.byref(r)) == da.E_ARG
    rng = (da.SeekRange * 1)()
    assert L.mi355_inflate_seek_read_batch_device(None, sp, rng, 1, None, None) == da.E_ARG
    assert L.mi355_inflate_seek_info(None, C.byref(da.SeekInfo())) == da.E_ARG
    n = C.c_size_t(0)
    assert L.mi355_inflate_seek_points(None, None, 0, C.byref(n)) == da.E_ARG
    assert L.mi355_inflate_seek_last_read(None, (C.c_uint64 * 4)()) == da.E_ARG
    L.mi355_inflate_seek_free(None)  # (like free)
