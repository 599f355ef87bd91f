"""ctypes binding of tests/infltable (host builds of the tabled inflate, inflate_table.h: the serial model and the three passes).
TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, E_OUT_TOO_SMALL, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "infltable")
LIB = os.path.join(DIR, "libinfltable.so")
FUZZ = os.path.join(DIR, "infltable_fuzz")

GROUP_DEFAULT = 256 << 20  # MI355_CFG_INFLATE_GROUP_BYTES's default
GROUP_MIN = 64 << 10       # ... and its minimum
TABLED_STATUS = [s for s in STATUS if s not in ("MISMATCH", "LENGTH")]  # what a tabled inflate can report

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.infltable_inflate.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64,
                                        C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.infltable_inflate.restype = C.c_int
        for name in ("unfenced_loads", "fences", "markers", "carry_depth", "groups"):
            getattr(L, "infltable_" + name).restype = C.c_uint64
        for name in ("report_size", "rec_size", "group_entries"):
            getattr(L, "infltable_" + name).restype = C.c_uint32
        L.infltable_reset_counters.restype = None
        _lib = L
    return _lib


def _arrays(table):
    n = len(table) if table else 0
    bits = (C.c_uint64 * max(n, 1))(*[t[0] for t in table or []])
    size = (C.c_uint64 * max(n, 1))(*[t[1] for t in table or []])
    return bits, size, n


def inflate(stream, wrapper=0, table=None, out_cap=0, three=True, group=GROUP_DEFAULT):
    """Returns (rc, out_len, report dict, the out_cap bytes of the buffer, canary intact?).  table: [(bit_start, in_bytes)] or None.
    three: the three passes as the kernels run them (else the serial model).  The buffer is out_cap bytes of 0xA5 with CANARY bytes of
    0xC3 behind them; out_cap == 0 hands the decoder a NULL buffer (the size query)."""
    buf = C.create_string_buffer(b"\xA5" * out_cap + b"\xC3" * CANARY, out_cap + CANARY) if out_cap else None
    bits, size, n = _arrays(table)
    r = Report()
    got = C.c_uint64(0)
    rc = lib().infltable_inflate(1 if three else 0, bytes(stream), len(stream), wrapper, bits, size, n, group,
                                 C.cast(buf, C.c_void_p) if out_cap else None, out_cap, C.byref(got), C.byref(r))
    raw = buf.raw if out_cap else b""
    return rc, got.value, report_dict(r), raw[:out_cap], raw[out_cap:] == b"\xC3" * CANARY if out_cap else True


def counters():
    L = lib()
    return dict(unfenced=L.infltable_unfenced_loads(), fences=L.infltable_fences(), markers=L.infltable_markers(),
                carry_depth=L.infltable_carry_depth(), groups=L.infltable_groups())


def reset_counters():
    lib().infltable_reset_counters()


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, table, group, out_cap) -- the file infltable_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"ITC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, table, group, cap in cases:
            f.write(struct.pack("<IQQQQ", wrapper, len(stream), cap, group, len(table)))
            for bit, n in table:
                f.write(struct.pack("<QQ", bit, n))
            f.write(bytes(stream))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
