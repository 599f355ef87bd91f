"""The inflate part of the C ABI (include/mi355_deflate.h) without a GPU: the report's layout in C and in ctypes, the new return
code, the header as C99, the mirror's names, the host twin's report.  CPU only."""
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
    int (*one)(mi355_deflate_ctx*, const void*, size_t, int, void*, size_t, size_t*, mi355_inflate_report*, void*) = 0;
    int (*host)(mi355_deflate_ctx*, const uint8_t*, size_t, int, uint8_t*, size_t, size_t*, mi355_inflate_report*) = 0;
    int (*batch)(mi355_deflate_ctx*, mi355_batch_item*, size_t, int, mi355_inflate_report*, void*) = 0;
    int same = sizeof(one == mi355_inflate_device) + sizeof(host == mi355_inflate) + sizeof(batch == mi355_inflate_batch_device);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(mi355_inflate_report), (int)offsetof(mi355_inflate_report, status),
           (int)offsetof(mi355_inflate_report, reserved), (int)offsetof(mi355_inflate_report, bit),
           (int)offsetof(mi355_inflate_report, out_pos), (int)offsetof(mi355_inflate_report, out_len),
           (int)offsetof(mi355_inflate_report, n_blocks), (int)offsetof(mi355_inflate_report, n_stored),
           (int)offsetof(mi355_inflate_report, n_fixed), (int)offsetof(mi355_inflate_report, n_dynamic),
           (int)offsetof(mi355_inflate_report, ms), MI355_E_DATA, same == 3 * (int)sizeof(int));
    return 0;
}
"""


def test_report_is_56_bytes_in_c_and_in_ctypes_and_the_header_is_c99(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    R = da.InflateReport
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_] + [da.E_DATA, 1]
    assert got[0] == 56 and got[-2] == -8


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in ("mi355_inflate", "mi355_inflate_device", "mi355_inflate_batch_device"):
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("inflate", "inflate_raw", "inflate_device", "inflate_batch_device"):
        assert callable(getattr(da.Context, name))
    assert callable(da.inflate_bytes)
    assert (da.E_DATA, da.E_OUT_TOO_SMALL) == (-8, -2)


def test_the_twins_report_is_the_abis():
    import deflate_amd as da
    import inflwrite_binding as iw
    assert iw.lib().inflwrite_report_size() == C.sizeof(da.InflateReport) == C.sizeof(iw.Report) == 56
    assert [f for f, _ in iw.Report._fields_] == [f for f, _ in da.InflateReport._fields_]
    assert iw.lib().inflwrite_rec_size() == 56  # what k_inflate leaves per stream
    assert iw.STATUS == da.VERIFY_STATUS and (iw.E_DATA, iw.E_OUT_TOO_SMALL) == (da.E_DATA, da.E_OUT_TOO_SMALL)
