"""The batched encode's C ABI without a GPU: the header declares it and compiles as C99, the library exports it, the
Python mirror has it, and the item lookup of the batched kernels' flat grids (stages.h batch_item_of) finds the right item."""
import os
import random
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
HEADER = os.path.join(ROOT, "include", "mi355_deflate.h")
STAGES = os.path.join(ROOT, "deflate-rs_amd", "csrc", "stages.h")
LIB = os.path.join(ROOT, "deflate-rs_amd", "libmi355deflate.so")
ENTRIES = ("mi355_deflate_encode_batch", "mi355_deflate_encode_batch_device", "mi355_deflate_last_batch_info")


def _cc():
    for c in ("gcc", "cc", "clang"):
        if subprocess.run(["which", c], capture_output=True).returncode == 0:
            return c
    pytest.skip("no C compiler")


def test_header_declares_the_batch_entries_and_structs():
    h = open(HEADER).read()
    for e in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % e, h), e
    assert re.search(r"}\s*mi355_batch_item\s*;", h)
    assert re.search(r"}\s*mi355_batch_info\s*;", h)
    item = h[h.index("typedef struct {\n    const void* in;"):h.index("} mi355_batch_item;")]
    for f in ("in", "in_len", "out", "out_cap", "out_len", "status"):
        assert re.search(r"\b%s;" % f, item), f


def test_library_exports_the_batch_entries():
    if not os.path.exists(LIB):
        pytest.skip("libmi355deflate.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for e in ENTRIES:
        assert e in syms, e


def test_python_mirror_has_the_batch_functions():
    import ctypes as C

    import deflate_amd as da
    for e in ENTRIES:
        assert e in da.EXPORTED
    for f in ("encode_batch", "encode_batch_device", "batch_info"):
        assert callable(getattr(da.Context, f))
    for f in ("deflate_bytes_batch_conf", "deflate_bytes_zlib_batch_conf", "deflate_bytes_batch", "deflate_bytes_zlib_batch"):
        assert callable(getattr(da, f))
    # the ctypes mirrors have the C layouts (x86-64: 8-byte pointers and size_t)
    assert C.sizeof(da.BatchItem) == 48
    assert C.sizeof(da.BatchInfo) == 48


def test_header_compiles_as_c99_pedantic(tmp_path):
    cc = _cc()
    src = tmp_path / "t.c"
    src.write_text('#include "mi355_deflate.h"\n#include <stddef.h>\n'
                   "_Static_assert(sizeof(mi355_batch_item) == 48, \"item\");\n"
                   "_Static_assert(offsetof(mi355_batch_info, n_batched) == 24, \"info\");\n"
                   "int main(void) { mi355_batch_item it = {0}; mi355_batch_info bi; (void)bi;\n"
                   "  int (*f)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*) = mi355_deflate_encode_batch;\n"
                   "  int (*g)(mi355_deflate_ctx*, mi355_batch_item*, size_t, const mi355_deflate_opts*, void*) = mi355_deflate_encode_batch_device;\n"
                   "  int (*h)(mi355_deflate_ctx*, mi355_batch_info*) = mi355_deflate_last_batch_info;\n"
                   "  (void)f; (void)g; (void)h; return it.status; }\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _prefix_items(pre):
    """plain walk over the running sums: the item of every workgroup in turn"""
    out = []
    for i in range(len(pre) - 1):
        out += [i] * (pre[i + 1] - pre[i])
    return out


def test_batch_item_lookup_matches_a_plain_search(tmp_path):
    gxx = None
    for c in ("g++", "c++", "clang++"):
        if subprocess.run(["which", c], capture_output=True).returncode == 0:
            gxx = c
            break
    if gxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "h.cpp"
    src.write_text('#include <cstdio>\n#include <cstdint>\n#include <vector>\n#include "stages.h"\n'
                   "int main() { unsigned n; std::vector<uint32_t> pre; std::vector<uint32_t> q;\n"
                   "  while (scanf(\"%u\", &n) == 1) { pre.resize(n + 1); for (auto& p : pre) scanf(\"%u\", &p);\n"
                   "    for (uint32_t bx = 0; bx < pre[n]; bx++) printf(\"%u \", mi355::batch_item_of(pre.data(), n, bx)); printf(\"\\n\"); }\n"
                   "  return 0; }\n")
    exe = tmp_path / "h"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-I", os.path.dirname(STAGES), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rnd = random.Random(7)
    cases = [[3], [0, 5], [5, 0], [0, 0, 1, 0], [1] * 64, [1] * 65, [2] * 4097, [0] * 100 + [1] + [0] * 100]
    for _ in range(40):
        n = rnd.choice([1, 2, 63, 64, 65, 200, 1000, 4100])
        cases.append([rnd.choice([0, 0, 1, 2, 3, 17, 40]) for _ in range(n)])
    cases = [c for c in cases if sum(c) > 0]
    text = ""
    pres = []
    for sizes in cases:
        pre = [0]
        for s in sizes:
            pre.append(pre[-1] + s)
        pres.append(pre)
        text += "%d %s\n" % (len(sizes), " ".join(map(str, pre)))
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(pres)
    for pre, line in zip(pres, out):
        got = list(map(int, line.split()))
        want = _prefix_items(pre)
        assert got == want
        for bx, i in enumerate(got):  # the item really has that workgroup
            assert pre[i] <= bx < pre[i + 1]
