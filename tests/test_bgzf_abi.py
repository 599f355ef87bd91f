"""The BGZF part of the C ABI (include/mi355_deflate.h) without a GPU: the four prototypes and the header as pedantic C99, the
library's exports, the mirror's names, mi355_bgzf_bound against the model, the argument errors, which are decided before the device
is touched, and the version, which stays where the other ABI tests pin it.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import bgzf_cases as bc

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "mi355_deflate.h"
int main(void) {
    /* the prototypes, compared inside sizeof: checked by the compiler, nothing to link */
    size_t (*bound)(size_t, size_t) = 0;
    int (*dev)(mi355_deflate_ctx*, const void*, size_t, const mi355_deflate_opts*, size_t, void*, size_t, size_t*, mi355_member_info*, size_t,
               size_t*, void*) = 0;
    int (*host)(mi355_deflate_ctx*, const uint8_t*, size_t, const mi355_deflate_opts*, size_t, uint8_t*, size_t, size_t*, mi355_member_info*,
                size_t, size_t*) = 0;
    int (*stages)(mi355_deflate_ctx*, float*) = 0;
    int same = sizeof(bound == mi355_bgzf_bound) + sizeof(dev == mi355_bgzf_encode_device) + sizeof(host == mi355_bgzf_encode) +
               sizeof(stages == mi355_bgzf_last_stages);
    printf("%d %d %d\n", MI355_DEFLATE_VERSION, (int)sizeof(mi355_member_info), same == 4 * (int)sizeof(int));
    return 0;
}
"""

NAMES = ("mi355_bgzf_bound", "mi355_bgzf_encode_device", "mi355_bgzf_encode", "mi355_bgzf_last_stages")


def test_the_header_declares_the_entries_and_is_c99_and_the_version_stays(tmp_path):
    src = os.path.join(str(tmp_path), "probe.c")
    exe = os.path.join(str(tmp_path), "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    assert subprocess.check_output([exe], universal_newlines=True).split() == ["101", "40", "1"]


def test_the_library_exports_the_entries_and_the_mirror_names_them():
    import deflate_amd as da
    L = da.load()
    for name in NAMES:
        assert name in da.EXPORTED
        assert getattr(L, name)
    assert L.mi355_deflate_version() == 101
    for name in ("encode_bgzf", "encode_bgzf_device", "bgzf_stages"):
        assert callable(getattr(da.Context, name))
    for name in ("bgzf_bound", "bgzf_bytes", "bgzf_gzi"):
        assert callable(getattr(da, name))
    assert da.BGZF_EOF == bc.EOF and da.BGZF_BLOCK_MAX == bc.BLOCK_MAX


def test_the_bound_needs_no_gpu_and_holds_every_model_file():
    import deflate_amd as da
    L = da.load()
    for c in bc.all_cases():
        file, _members = bc.model(c.data, c.level, c.block)
        b = da.bgzf_bound(len(c.data), c.block)
        lens = [len(s) for s in bc.slices(c.data, c.block)]
        assert b == sum(L.mi355_deflate_bound_ex(n, 2, 18, 0) for n in lens) + 28
        assert b >= len(file), c.name
    assert da.bgzf_bound(0) == 28 and da.bgzf_bound(10, 65281) == 0 and da.bgzf_bound(10, 65280) == da.bgzf_bound(10, 0) == da.bgzf_bound(10)
    assert da.bgzf_bound(10, 1) == 10 * L.mi355_deflate_bound_ex(1, 2, 18, 0) + 28


def test_argument_errors_are_decided_before_the_device_is_touched():
    """no context can be made here, so the one handed over is a block of zeros that a call would have to read to get any further:
    every case below is refused on its arguments alone"""
    import deflate_amd as da
    L = da.load()
    fake = (C.c_uint8 * 65536)()
    ctx = C.cast(fake, C.c_void_p)
    o = da.CompressionOptions.default().to_c(2, 0, 0)
    n, nm = C.c_size_t(7), C.c_size_t(7)
    tab = (da.MemberInfo * 2)()
    buf = (C.c_uint8 * 96)()
    base = C.addressof(buf)
    out = C.c_void_p((base + 15) & ~15)
    for host in (True, False):
        fn = L.mi355_bgzf_encode if host else L.mi355_bgzf_encode_device
        tail = () if host else (None,)
        s = b"12345678" if host else out
        assert fn(None, s, 8, C.byref(o), 0, out, 64, C.byref(n), tab, 2, C.byref(nm), *tail) == da.E_ARG      # no context
        assert fn(ctx, s, 8, None, 0, out, 64, C.byref(n), tab, 2, C.byref(nm), *tail) == da.E_ARG              # no options
        assert fn(ctx, s, 8, C.byref(o), 0, out, 64, None, tab, 2, C.byref(nm), *tail) == da.E_ARG              # no out_len
        assert fn(ctx, s, 8, C.byref(o), 65281, out, 64, C.byref(n), tab, 2, C.byref(nm), *tail) == da.E_ARG    # block_size
        assert fn(ctx, None, 8, C.byref(o), 0, out, 64, C.byref(n), tab, 2, C.byref(nm), *tail) == da.E_ARG     # bytes without an input
        assert fn(ctx, s, 8, C.byref(o), 0, None, 64, C.byref(n), tab, 2, C.byref(nm), *tail) == da.E_ARG       # room without a buffer
        assert fn(ctx, s, 8, C.byref(o), 0, out, 64, C.byref(n), None, 2, C.byref(nm), *tail) == da.E_ARG       # table room without a table
    odd = C.c_void_p(out.value + 4)
    assert L.mi355_bgzf_encode_device(ctx, out, 8, C.byref(o), 0, odd, 64, C.byref(n), tab, 2, C.byref(nm), None) == da.E_ARG  # d_out & 15
    assert (n.value, nm.value) == (7, 7) and bytes(fake) == bytes(65536)
    assert L.mi355_bgzf_last_stages(None, None) == da.E_ARG
    assert L.mi355_bgzf_last_stages(ctx, None) == da.E_ARG
