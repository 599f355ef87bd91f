"""The packed batch's C ABI without a GPU: the header declares the three entries and mi355_packed_entry and compiles as C99,
the library exports them, the Python mirror has them, and mi355_deflate_batch_packed_bound -- which needs no GPU -- is the sum
of the items' aligned bounds."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
HEADER = os.path.join(ROOT, "include", "mi355_deflate.h")
LIB = os.path.join(ROOT, "deflate-rs_amd", "libmi355deflate.so")
ENTRIES = ("mi355_deflate_batch_packed_bound", "mi355_deflate_encode_batch_packed", "mi355_deflate_encode_batch_packed_device")


def _cc():
    for c in ("gcc", "cc", "clang"):
        if subprocess.run(["which", c], capture_output=True).returncode == 0:
            return c
    pytest.skip("no C compiler")


def align_up(v, a):
    return (v + a - 1) // a * a


def test_header_declares_the_packed_entries():
    h = open(HEADER).read()
    assert re.search(r"\bsize_t\s+mi355_deflate_batch_packed_bound\s*\(", h)
    for e in ENTRIES[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % e, h), e
    assert re.search(r"}\s*mi355_packed_entry\s*;", h)
    assert re.search(r"#define\s+MI355_DEFLATE_VERSION\s+101\b", h)


def test_library_exports_the_packed_entries():
    if not os.path.exists(LIB):
        pytest.skip("libmi355deflate.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for e in ENTRIES:
        assert e in syms, e


def test_python_mirror_has_the_packed_functions():
    import deflate_amd as da
    L = da.load()
    for e in ENTRIES:
        assert e in da.EXPORTED
        getattr(L, e)
    assert L.mi355_deflate_version() >= 101
    for f in ("encode_batch_packed", "encode_batch_packed_device"):
        assert callable(getattr(da.Context, f))
    for f in ("packed_bound", "deflate_bytes_batch_packed_conf", "deflate_bytes_batch_packed"):
        assert callable(getattr(da, f))
    assert C.sizeof(da.PackedEntry) == 24
    assert (da.PackedEntry.off.offset, da.PackedEntry.len.offset, da.PackedEntry.status.offset) == (0, 8, 16)


def test_header_compiles_as_c99_pedantic_with_the_entry_layout(tmp_path):
    cc = _cc()
    src = tmp_path / "t.c"
    src.write_text('#include "mi355_deflate.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(mi355_packed_entry) == 24, \"entry\");\n"
                   "_Static_assert(offsetof(mi355_packed_entry, off) == 0, \"off\");\n"
                   "_Static_assert(offsetof(mi355_packed_entry, len) == 8, \"len\");\n"
                   "_Static_assert(offsetof(mi355_packed_entry, status) == 16, \"status\");\n"
                   "int main(void) { mi355_packed_entry e = {0};\n"
                   "  size_t (*b)(const mi355_batch_item*, size_t, int, const mi355_gzip_header*, size_t, size_t) =\n"
                   "      mi355_deflate_batch_packed_bound;\n"
                   "  int (*f)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*, const mi355_gzip_header*, size_t,\n"
                   "           uint8_t*, size_t, size_t, size_t*) = mi355_deflate_encode_batch_packed;\n"
                   "  int (*g)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*, const mi355_gzip_header*, size_t,\n"
                   "           void*, size_t, size_t, mi355_packed_entry*, size_t*, void*) = mi355_deflate_encode_batch_packed_device;\n"
                   "  (void)b; (void)f; (void)g; return e.status; }\n")
    r = subprocess.run([cc, "-std=c11", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (the header itself stays C99: _Static_assert is the only C11 word above)
    src2 = tmp_path / "u.c"
    src2.write_text('#include "mi355_deflate.h"\nint main(void) { mi355_packed_entry e = {0}; return e.status; }\n')
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src2),
                        "-o", str(tmp_path / "u.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


LENS = [0, 1, 2, 3, 4, 5, 100, 4093, 31744, 32767, 65536, 200001, (2 << 20) + 1]


@pytest.mark.parametrize("align", [4, 8, 4096])
def test_packed_bound_is_the_sum_of_the_aligned_bounds(align):
    if not os.path.exists(LIB):
        pytest.skip("libmi355deflate.so not built")
    import deflate_amd as da
    L = da.load()
    n = len(LENS)
    h_even = da.gzip_header(filename=b"six.bin")  # 10 + 7 + 1 = 18 bytes
    h_odd = da.gzip_header(filename=b"eight.bi")  # 19 bytes
    assert len(h_even) % 2 == 0 and len(h_odd) % 2 == 1
    per_item = [da.gzip_header(filename=b"n" * (k + 1)) for k in range(n)]  # odd and even lengths in turn
    assert {len(h) % 2 for h in per_item} == {0, 1}
    cases = [(0, None, [0] * n), (1, None, [0] * n), (2, None, [10] * n), (2, h_even, [len(h_even)] * n), (2, h_odd, [len(h_odd)] * n),
             (2, per_item, [len(h) for h in per_item])]
    for wrapper, headers, hlens in cases:
        want = sum(align_up(L.mi355_deflate_bound_ex(ln, wrapper, hl, 0), align) for ln, hl in zip(LENS, hlens))
        assert da.packed_bound(LENS, wrapper, headers, align) == want, (wrapper, hlens[:2])
        assert da.packed_bound([], wrapper, None if isinstance(headers, list) else headers, align) == 0
    # headers are read for wrapper 2 only
    assert da.packed_bound(LENS, 1, per_item, align) == da.packed_bound(LENS, 1, None, align)
    # align 0 means 4
    assert da.packed_bound(LENS, 0, None, 0) == da.packed_bound(LENS, 0, None, 4)
