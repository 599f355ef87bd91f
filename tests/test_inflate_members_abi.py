"""The members part of the C ABI (include/mi355_deflate.h) without a GPU: the prototypes and the member row's layout in C and in
ctypes, the header as C99, the setting's number, the mirror's names, the host twin's row, and the argument errors, which are decided
before a context or the device is touched.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "mi355_deflate.h"
int main(void) {
    /* the prototypes, compared inside sizeof: checked by the compiler, nothing to link */
    int (*dev)(mi355_deflate_ctx*, const void*, size_t, void*, size_t, size_t*, mi355_member_info*, size_t, size_t*, mi355_inflate_report*,
               void*) = 0;
    int (*host)(mi355_deflate_ctx*, const uint8_t*, size_t, uint8_t*, size_t, size_t*, mi355_member_info*, size_t, size_t*,
                mi355_inflate_report*) = 0;
    int (*stages)(mi355_deflate_ctx*, float*) = 0;
    int (*walks)(mi355_deflate_ctx*, uint64_t*, mi355_member_walk*, size_t, size_t*) = 0;
    int same = sizeof(dev == mi355_inflate_members_device) + sizeof(host == mi355_inflate_members) +
               sizeof(stages == mi355_inflate_members_last_stages) + sizeof(walks == mi355_inflate_members_last_walks);
    if (sizeof(mi355_member_walk) != 40 || offsetof(mi355_member_walk, end) != 8 || offsetof(mi355_member_walk, n_members) != 16 ||
        offsetof(mi355_member_walk, out_bytes) != 24 || offsetof(mi355_member_walk, how) != 32 || offsetof(mi355_member_walk, link) != 36)
        return 1;
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(mi355_member_info), (int)offsetof(mi355_member_info, in_off),
           (int)offsetof(mi355_member_info, in_len), (int)offsetof(mi355_member_info, out_off), (int)offsetof(mi355_member_info, out_len),
           (int)offsetof(mi355_member_info, flags), (int)offsetof(mi355_member_info, status), MI355_CFG_INFLATE_MEMBER_SPAN_BYTES,
           (int)MI355_MEMBER_HINTED, same == 4 * (int)sizeof(int));
    return 0;
}
"""


def test_member_info_is_40_bytes_in_c_and_in_ctypes_and_the_header_is_c99(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    M = da.MemberInfo
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f, _ in M._fields_] + [da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, da.MEMBER_HINTED, 1]
    assert got[0] == 40 and got[-3] == 13 and got[-2] == 1


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in ("mi355_inflate_members", "mi355_inflate_members_device", "mi355_inflate_members_last_stages",
                 "mi355_inflate_members_last_walks"):
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("inflate_members", "inflate_members_raw", "inflate_members_device", "inflate_members_stages", "inflate_members_walks"):
        assert callable(getattr(da.Context, name))
    for kw in (dict(wrapper=0), dict(wrapper=1), dict(wrapper=2, parallel=True), dict(wrapper=2, blocks=[])):
        with pytest.raises(ValueError):
            da.inflate_bytes(b"", members=True, **kw)


def test_the_twins_row_is_the_abis():
    import deflate_amd as da
    import inflmembers_binding as mb
    assert mb.lib().inflmembers_member_size() == C.sizeof(da.MemberInfo) == C.sizeof(mb.Member) == 40
    assert [f for f, _ in mb.Member._fields_] == [f for f, _ in da.MemberInfo._fields_]
    assert C.sizeof(da.MemberWalk) == C.sizeof(mb.Walk) == 40 and da.MemberWalk._fields_ == mb.Walk._fields_
    assert mb.HINTED == da.MEMBER_HINTED and (mb.span_min(), mb.span_default()) == (16, 65536)


def test_argument_errors_are_decided_before_a_context_is_touched():
    import deflate_amd as da
    L = da.load()
    n, nm, r = C.c_size_t(0), C.c_size_t(0), da.InflateReport()
    tab = (da.MemberInfo * 2)()
    buf = (C.c_uint8 * 8)()
    out = C.cast(buf, C.c_void_p)
    for host in (True, False):
        fn = L.mi355_inflate_members if host else L.mi355_inflate_members_device
        tail = () if host else (None,)
        s = b"12345678" if host else out
        assert fn(None, s, 8, out, 8, None, tab, 2, C.byref(nm), C.byref(r), *tail) == da.E_ARG            # no out_len
        assert fn(None, s, 8, out, 8, C.byref(n), tab, 2, C.byref(nm), None, *tail) == da.E_ARG           # no report
        assert fn(None, None, 8, out, 8, C.byref(n), tab, 2, C.byref(nm), C.byref(r), *tail) == da.E_ARG  # bytes without a stream
        assert fn(None, s, 8, None, 8, C.byref(n), tab, 2, C.byref(nm), C.byref(r), *tail) == da.E_ARG    # room without a buffer
        assert fn(None, s, 8, out, 8, C.byref(n), None, 2, C.byref(nm), C.byref(r), *tail) == da.E_ARG    # table room without a table
    assert L.mi355_inflate_members_last_stages(None, None) == da.E_ARG
    assert L.mi355_inflate_members_last_walks(None, None, None, 0, C.byref(n)) == da.E_ARG
    for bad in (0, 15, (1 << 30) + 1):  # the span setting's range, refused before the default context would be made
        assert L.mi355_deflate_ctx_config(None, da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, bad) == da.E_ARG
