"""The cuts' part of the C ABI (include/mi355_deflate.h) without a GPU: the key, the prototypes and the record as C99, the mirror's
names and structure, the host build's records, the key's range and the argument errors of the three calls, which are decided before
a context or the device is touched.  CPU only."""
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
    int (*cuts)(mi355_inflate_seek*, mi355_seek_cut*, size_t, size_t*) = 0;
    int (*info)(mi355_inflate_seek*, uint64_t*) = 0;
    int (*last)(mi355_inflate_seek*, uint64_t*) = 0;
    int (*stages)(mi355_deflate_ctx*, float*) = 0;
    int (*get)(mi355_deflate_ctx*, int, uint64_t*) = 0;
    int same = sizeof(cuts == mi355_inflate_seek_cuts) + sizeof(info == mi355_inflate_seek_cut_info) +
               sizeof(last == mi355_inflate_seek_last_read_cuts) + sizeof(stages == mi355_inflate_seek_last_read_stages) +
               sizeof(get == mi355_deflate_ctx_config_get) + 0 * MI355_CFG_INFLATE_SEEK_CUT_WALKER;
    printf("%d %d %d %d %d %d\n", MI355_CFG_INFLATE_SEEK_CUT_BYTES, (int)sizeof(mi355_seek_cut), (int)offsetof(mi355_seek_cut, bit),
           (int)offsetof(mi355_seek_cut, pos), (int)offsetof(mi355_seek_cut, hdr_bit), same == 5 * (int)sizeof(int));
    return 0;
}
"""

NAMES = ("mi355_inflate_seek_cuts", "mi355_inflate_seek_cut_info", "mi355_inflate_seek_last_read_cuts", "mi355_inflate_seek_last_read_stages",
         "mi355_deflate_ctx_config_get")


def test_the_header_is_c99_and_names_the_key_and_the_entry_points(tmp_path):
    import deflate_amd as da
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(x) for x in subprocess.check_output([exe], universal_newlines=True).split()]
    assert got == [da.Context.CFG_INFLATE_SEEK_CUT_BYTES, C.sizeof(da.SeekCut), da.SeekCut.bit.offset, da.SeekCut.pos.offset,
                   da.SeekCut.hdr_bit.offset, 1]
    assert got[:2] == [15, 24]


def test_the_mirror_names_the_entry_points():
    import deflate_amd as da
    for name in NAMES:
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("cuts", "cut_info", "last_read_cuts"):
        assert callable(getattr(da.SeekIndex, name))
    import inspect
    for name in ("inflate_seek", "inflate_seek_device"):
        assert inspect.signature(getattr(da.Context, name)).parameters["cut"].default == 0


def test_the_keys_range_is_judged_before_the_device():
    """ctx NULL: were the device touched, a machine without one would answer MI355_E_HIP"""
    import deflate_amd as da
    L = da.load()
    for value in (1, 63, (1 << 30) + 1, 1 << 31, (1 << 64) - 1):
        assert L.mi355_deflate_ctx_config(None, 15, value) == da.E_ARG
    v = C.c_uint64(0)
    assert L.mi355_deflate_ctx_config(None, 16, 2) in (da.E_ARG, da.E_HIP)  # (0 or 1: judged with the context in hand)
    for key in (0, 10, 17):
        assert L.mi355_deflate_ctx_config_get(None, key, C.byref(v)) == da.E_ARG
    assert L.mi355_deflate_ctx_config_get(None, 15, None) == da.E_ARG


def test_argument_errors_come_before_the_device():
    import deflate_amd as da
    L = da.load()
    n = C.c_size_t(0)
    v = (C.c_uint64 * 4)()
    one = (da.SeekCut * 1)()
    assert L.mi355_inflate_seek_cuts(None, None, 0, C.byref(n)) == da.E_ARG
    assert L.mi355_inflate_seek_cuts(None, one, 1, C.byref(n)) == da.E_ARG
    assert L.mi355_inflate_seek_cut_info(None, v) == da.E_ARG
    assert L.mi355_inflate_seek_last_read_cuts(None, v) == da.E_ARG
    assert L.mi355_inflate_seek_last_read_stages(None, None) == da.E_ARG


def test_the_host_build_accepts_the_keys_range_only():
    import inflate_cut_cases as cc
    import inflcut_binding as cb
    c = cc.by_name("stored/w0")
    for cut in (1, 63, (1 << 30) + 1):
        assert cb.Index(c.stream, 0, c.table, cc.SPACING, cut=cut).rc == cb.E_ARG
    for cut in (0, 64, 1 << 30):
        assert cb.Index(c.stream, 0, c.table, cc.SPACING, cut=cut).rc == cb.OK
