"""The tabled-inflate part of the C ABI (include/mi355_deflate.h) without a GPU: the prototypes and the new setting as C99, the
mirror's names, the host builds' records, and the argument errors of a tabled call, which are decided before a context or the device
is touched.  CPU only."""
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
    int (*dev)(mi355_deflate_ctx*, const void*, size_t, int, const mi355_block_info*, size_t, void*, size_t, size_t*,
               mi355_inflate_report*, void*) = 0;
    int (*host)(mi355_deflate_ctx*, const uint8_t*, size_t, int, const mi355_block_info*, size_t, uint8_t*, size_t, size_t*,
                mi355_inflate_report*) = 0;
    int same = sizeof(dev == mi355_inflate_tabled_device) + sizeof(host == mi355_inflate_tabled);
    printf("%d %d %d %d %d %d\n", (int)sizeof(mi355_inflate_report), (int)sizeof(mi355_block_info),
           (int)offsetof(mi355_block_info, in_bytes), (int)offsetof(mi355_block_info, bit_start), MI355_CFG_INFLATE_GROUP_BYTES,
           same == 2 * (int)sizeof(int));
    return 0;
}
"""


def test_the_header_is_c99_and_names_the_entry_points_and_the_setting(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    B = da.BlockInfo
    assert got == [C.sizeof(da.InflateReport), C.sizeof(B), B.in_bytes.offset, B.bit_start.offset, da.Context.CFG_INFLATE_GROUP_BYTES, 1]
    assert got[0] == 56 and got[4] == 11


def test_the_mirror_names_the_entry_points():
    import inspect

    import deflate_amd as da
    for name in ("mi355_inflate_tabled", "mi355_inflate_tabled_device", "mi355_inflate_tabled_last_stages"):
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for fn in (da.Context.inflate, da.Context.inflate_raw, da.Context.inflate_device, da.inflate_bytes):
        assert inspect.signature(fn).parameters["blocks"].default is None
    assert "TABLE" in da.VERIFY_STATUS


def test_the_host_builds_records_are_the_abis():
    import deflate_amd as da
    import infltable_binding as tb
    L = tb.lib()
    assert L.infltable_report_size() == C.sizeof(da.InflateReport) == C.sizeof(tb.Report) == 56
    assert L.infltable_rec_size() == 56  # what k_inflate_tab leaves per entry
    assert L.infltable_group_entries() == 4096
    assert tb.STATUS == da.VERIFY_STATUS and (tb.E_DATA, tb.E_OUT_TOO_SMALL, tb.E_ARG) == (da.E_DATA, da.E_OUT_TOO_SMALL, da.E_ARG)
    assert (tb.GROUP_DEFAULT, tb.GROUP_MIN) == (256 << 20, 64 << 10)


def test_argument_errors_of_a_tabled_call_come_before_the_device():
    """ctx NULL: were the device touched, a machine without one would answer MI355_E_HIP"""
    import deflate_amd as da
    L = da.load()
    n, r = C.c_size_t(0), da.InflateReport()
    s = C.create_string_buffer(b"\x03\x00", 2)
    sp = C.cast(s, C.c_void_p)
    out = C.create_string_buffer(16)
    op = C.cast(out, C.c_void_p)

    def table(*pairs):
        arr = (da.BlockInfo * len(pairs))()
        for k, (bit, size) in enumerate(pairs):
            arr[k].bit_start, arr[k].in_bytes = bit, size
        return arr

    one = table((0, 0))
    for fn, sarg, oarg in ((L.mi355_inflate_tabled_device, sp, op), (L.mi355_inflate_tabled, s.raw, op)):
        tail = (None,) if fn is L.mi355_inflate_tabled_device else ()
        assert fn(None, sarg, 2, 3, one, 1, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG   # wrapper
        assert fn(None, sarg, 2, -1, one, 1, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, None, 2, 0, one, 1, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG   # a length without a stream
        assert fn(None, sarg, 2, 0, one, 1, None, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG   # a size without a buffer
        assert fn(None, sarg, 2, 0, one, 1, oarg, 16, None, C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, one, 1, oarg, 16, C.byref(n), None, *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, table((8, 0), (0, 0)), 2, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG  # bits descend
        assert fn(None, sarg, 2, 0, table((1, 0)), 1, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG  # the first entry not at bit 0
        assert fn(None, sarg, 2, 0, table((8, 0), (16, 0)), 2, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
        assert fn(None, sarg, 2, 0, table((0, 1 << 63), (0, 1 << 63)), 2, oarg, 16, C.byref(n), C.byref(r), *tail) == da.E_ARG
