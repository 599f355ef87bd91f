"""The verify part of the C ABI (include/mi355_deflate.h) without a GPU: the report's layout in C and in ctypes, the new return
code, the header as C99.  CPU only."""
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
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(mi355_verify_report), (int)offsetof(mi355_verify_report, status),
           (int)offsetof(mi355_verify_report, entry), (int)offsetof(mi355_verify_report, bit), (int)offsetof(mi355_verify_report, in_pos),
           (int)offsetof(mi355_verify_report, n_blocks), (int)offsetof(mi355_verify_report, n_stored),
           (int)offsetof(mi355_verify_report, n_fixed), (int)offsetof(mi355_verify_report, n_dynamic),
           (int)offsetof(mi355_verify_report, ms), MI355_E_VERIFY);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", MI355_VERIFY_OK, MI355_VERIFY_FRAME, MI355_VERIFY_BTYPE, MI355_VERIFY_STORED,
           MI355_VERIFY_LENGTHS, MI355_VERIFY_CODE, MI355_VERIFY_DISTANCE, MI355_VERIFY_MISMATCH, MI355_VERIFY_LENGTH,
           MI355_VERIFY_TABLE, MI355_VERIFY_TRUNCATED, MI355_VERIFY_TRAILER, MI355_VERIFY_CHECKSUM);
    return 0;
}
"""


def test_report_is_48_bytes_in_c_and_in_ctypes_and_the_header_is_c99(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    lines = subprocess.check_output([exe], universal_newlines=True).splitlines()
    got = [int(x) for x in lines[0].split()]
    R = da.VerifyReport
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_] + [da.E_VERIFY]
    assert got[0] == 48 and got[-1] == -7
    assert [int(x) for x in lines[1].split()] == list(range(13)) and len(da.VERIFY_STATUS) == 13


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in ("mi355_deflate_verify", "mi355_deflate_verify_device", "mi355_deflate_verify_batch_device"):
        assert name in da.EXPORTED
    assert da.load().mi355_deflate_version() == 101
    for name in ("verify", "verify_device", "verify_batch_device"):
        assert callable(getattr(da.Context, name))
    assert callable(da.verify_bytes)


def test_the_twins_report_is_the_abis():
    import deflate_amd as da
    import inflcheck_binding as ib
    assert ib.lib().inflcheck_report_size() == C.sizeof(da.VerifyReport) == C.sizeof(ib.Report) == 48
    assert ib.STATUS == da.VERIFY_STATUS and ib.E_VERIFY == da.E_VERIFY
