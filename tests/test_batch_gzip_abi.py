"""CPU-only: the gzip forms of the batched encode (mi355_deflate_encode_batch[_device]_gzip, mi355_gzip_header) are declared in
include/mi355_deflate.h as plain C with the agreed signatures, exported by the library and mirrored by deflate_amd."""
import ctypes as C
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

ENTRIES = ("mi355_deflate_encode_batch_gzip", "mi355_deflate_encode_batch_device_gzip")

PROBE = r"""
#include "mi355_deflate.h"
typedef char size_is_16[sizeof(mi355_gzip_header) == 16 ? 1 : -1];
int main(void) {
    int (*host)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*, const mi355_gzip_header*, size_t) =
        mi355_deflate_encode_batch_gzip;
    int (*dev)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*, const mi355_gzip_header*, size_t, void*) =
        mi355_deflate_encode_batch_device_gzip;
    mi355_gzip_header h;
    const uint8_t* p = 0;
    size_t n = 0;
    h.hdr = p;
    h.hdr_len = n;
    return (host != 0 && dev != 0 && h.hdr == 0 && h.hdr_len == 0) ? 0 : 1;
}
"""


def header_text():
    return open(os.path.join(ROOT, "include", "mi355_deflate.h")).read()


def test_header_declares_the_entries_and_the_struct():
    hdr = header_text()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert re.search(r"typedef\s+struct\s*\{[^}]*\bhdr\b[^}]*\bhdr_len\b[^}]*\}\s*mi355_gzip_header\s*;", hdr, flags=re.S)
    # the comment over them names what they mirror
    assert "src/lib.rs:242-267" in hdr[hdr.index("mi355_deflate_last_batch_info("):hdr.index("mi355_deflate_encode_batch_gzip(")]


def test_header_compiles_as_c99_with_the_exact_signatures(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
           str(tmp_path / "probe.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_both_symbols():
    import deflate_amd
    nm = subprocess.run(["nm", "-D", "--defined-only", deflate_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TDB] (mi355_[a-z0-9_]+)$", nm, flags=re.M))
    for name in ENTRIES:
        assert name in exported, name


def test_python_mirror():
    import deflate_amd as da
    L = da.load()
    for name in ENTRIES:
        assert name in da.EXPORTED, name
        assert getattr(L, name).argtypes is not None, name
    assert C.sizeof(da.GzipHeader) == 16
    assert [f[0] for f in da.GzipHeader._fields_] == ["hdr", "hdr_len"]
    assert len(L.mi355_deflate_encode_batch_gzip.argtypes) == 6
    assert len(L.mi355_deflate_encode_batch_device_gzip.argtypes) == 7
    for name in ("encode_batch_gzip", "encode_batch_device_gzip"):
        assert callable(getattr(da.Context, name)), name
    for name in ("deflate_bytes_gzip_batch_conf", "deflate_bytes_gzip_batch"):
        assert callable(getattr(da, name)), name
