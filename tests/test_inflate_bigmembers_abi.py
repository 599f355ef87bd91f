"""The large plain members' part of the C ABI (include/mi355_deflate.h) without a GPU: the new setting and the two measuring aids in
the header as C99, in the library's exports and in the Python mirror; the setting's range, refused before a context or the device is
touched; the host twin's constants.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

PROBE = r"""
#include <stdio.h>
#include "mi355_deflate.h"
int main(void) {
    /* the prototypes, compared inside sizeof: checked by the compiler, nothing to link */
    int (*par)(mi355_deflate_ctx*, uint64_t*) = 0;
    int (*stages)(mi355_deflate_ctx*, float*) = 0;
    int same = sizeof(par == mi355_inflate_members_last_parallel) + sizeof(stages == mi355_inflate_members_last_parallel_stages);
    printf("%d %d\n", MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES, same == 2 * (int)sizeof(int));
    return 0;
}
"""


def test_the_header_declares_the_setting_and_the_aids_as_c99(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    assert subprocess.check_output([exe], universal_newlines=True).split() == ["14", "1"]
    text = open(os.path.join(ROOT, "include", "mi355_deflate.h")).read()
    at = text.index("MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES  ")
    para = text[at: text.index("*/", at)]
    assert "Same results either way" in para and "not measured" in para and "0 switches the path off" in para


def test_the_library_and_the_mirror_name_them():
    import deflate_amd as da
    assert da.Context.CFG_INFLATE_MEMBER_PARALLEL_BYTES == 14
    for name in ("mi355_inflate_members_last_parallel", "mi355_inflate_members_last_parallel_stages"):
        assert name in da.EXPORTED
        assert getattr(da.load(), name)
    for name in ("inflate_members_last_parallel", "inflate_members_parallel_stages"):
        assert callable(getattr(da.Context, name))


def test_the_settings_range_is_decided_before_a_context_is_touched():
    import deflate_amd as da
    L = da.load()
    key = da.Context.CFG_INFLATE_MEMBER_PARALLEL_BYTES
    for bad in (1, 1023, (1 << 30) + 1, 1 << 40):
        assert L.mi355_deflate_ctx_config(None, key, bad) == da.E_ARG
    # 0 (off), both ends of the range and the default are no argument errors (without a device the default context cannot be made)
    for good in (0, 1024, 1 << 16, 1 << 30):
        assert L.mi355_deflate_ctx_config(None, key, good) in (da.OK, da.E_HIP)
    assert L.mi355_inflate_members_last_parallel(None, None) == da.E_ARG
    assert L.mi355_inflate_members_last_parallel_stages(None, None) == da.E_ARG


def test_the_twins_constants_are_the_settings():
    import inflbig_binding as bb
    L = bb.lib()
    assert L.inflbig_par_default() == 65536 == 4 * 16384  # four index spans at their default
    assert L.inflbig_part_size() == 72
    assert (bb.first_extent(1024, 256), bb.first_extent(1024, 4096), bb.first_extent(65536, 16384)) == (4, 1, 4)
    assert L.inflbig_set(1023, 256, 65536) == bb.E_ARG and L.inflbig_set(0, 256, 65536) == bb.OK
    assert C.sizeof(bb.Member) == 40
