"""ctypes binding of tests/inflcheck (host build of the verify decisions, inflate_check.h).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflcheck")
LIB = os.path.join(DIR, "libinflcheck.so")
FUZZ = os.path.join(DIR, "inflcheck_fuzz")

STATUS = ["OK", "FRAME", "BTYPE", "STORED", "LENGTHS", "CODE", "DISTANCE", "MISMATCH", "LENGTH", "TABLE", "TRUNCATED", "TRAILER",
          "CHECKSUM"]
OK, E_ARG, E_VERIFY = 0, -1, -7


class Report(C.Structure):
    _fields_ = [("status", C.c_uint32), ("entry", C.c_uint32), ("bit", C.c_uint64), ("in_pos", C.c_uint64),
                ("n_blocks", C.c_uint64), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32), ("n_dynamic", C.c_uint32),
                ("ms", C.c_float)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.inflcheck_verify.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(Report)]
        L.inflcheck_verify.restype = C.c_int
        L.inflcheck_verify_lanes.argtypes = L.inflcheck_verify.argtypes
        L.inflcheck_verify_lanes.restype = C.c_int
        L.inflcheck_match_token.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                            C.POINTER(C.c_uint32)]
        L.inflcheck_match_token.restype = None
        L.inflcheck_report_size.restype = C.c_uint32
        L.inflcheck_tables_size.restype = C.c_uint32
        _lib = L
    return _lib


def verify(stream, data, wrapper=0, table=None, lanes=False):
    """table: [(bit_start, in_bytes), ...] or None.  Returns (rc, dict of the report with the status as a name).
    lanes: compare bytes the kernel's way, 64 lanes at a time (the same report)"""
    n = len(table) if table else 0
    bs = (C.c_uint64 * max(n, 1))(*[t[0] for t in (table or [])])
    ib = (C.c_uint64 * max(n, 1))(*[t[1] for t in (table or [])])
    r = Report()
    rc = (lib().inflcheck_verify_lanes if lanes else lib().inflcheck_verify)(bytes(stream), len(stream), bytes(data), len(data), wrapper, bs, ib, n, C.byref(r))
    return rc, dict(status=STATUS[r.status] if r.status < len(STATUS) else r.status, entry=r.entry, bit=r.bit, in_pos=r.in_pos,
                    n_blocks=r.n_blocks, n_stored=r.n_stored, n_fixed=r.n_fixed, n_dynamic=r.n_dynamic)


def match_token(dist_lens, w, s, used, avail, p):
    """ic_match_token under the distance set of the 32 code lengths `dist_lens`: w holds the token's bits from the length symbol's
    code on (bit 0 first), used the bits of that code, avail the bits inside the stream.  Returns (status name, len, dist, used)."""
    assert len(dist_lens) == 32
    out = (C.c_uint32 * 4)()
    lib().inflcheck_match_token(bytes(dist_lens), w, s, used, avail, p, out)
    return STATUS[out[0]] if out[0] < len(STATUS) else out[0], out[1], out[2], out[3]


def write_corpus(path, cases):
    """cases: iterable of (stream, data, wrapper) or (stream, data, wrapper, table) -- the file inflcheck_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"IFC1" + struct.pack("<I", len(cases)))
        for c in cases:
            stream, data, wrapper = c[0], c[1], c[2]
            table = c[3] if len(c) > 3 and c[3] else []
            f.write(struct.pack("<IQQQ", wrapper, len(stream), len(data), len(table)))
            f.write(bytes(stream))
            f.write(bytes(data))
            for b, n in table:
                f.write(struct.pack("<QQ", b, n))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
