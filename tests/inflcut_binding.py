"""ctypes binding of tests/inflcut (host build of the cuts of a seek handle, inflate_cut.h: the build with its cut list, a read as its
plan, one turn per cut, flatten and the passes of inflate_seek.h, in two forms, and the three mutants).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflcut")
LIB = os.path.join(DIR, "libinflcut.so")
FUZZ = os.path.join(DIR, "inflcut_fuzz")

GROUP_DEFAULT = 256 << 20  # MI355_CFG_INFLATE_GROUP_BYTES's default
GROUP_MIN = 64 << 10       # ... and its minimum
MUTANT_RULE, MUTANT_INSIDE, MUTANT_STOP = 1, 2, 3
FILL = 0xA5
COUNTS = ("entries", "symbols", "steps", "sets")
CUT_COUNTS = ("cuts", "symbols", "steps", "launches")

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        u64p = C.POINTER(C.c_uint64)
        L.inflcut_build.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_int, u64p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                    C.POINTER(C.c_int), C.POINTER(Report)]
        L.inflcut_build.restype = C.c_void_p
        L.inflcut_free.argtypes = [C.c_void_p]
        L.inflcut_free.restype = None
        L.inflcut_info.argtypes = [C.c_void_p, u64p]
        L.inflcut_info.restype = None
        L.inflcut_cuts.argtypes = [C.c_void_p, u64p, C.c_uint64]
        L.inflcut_cuts.restype = C.c_uint64
        L.inflcut_set_cut.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
        L.inflcut_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, u64p, u64p, u64p, C.c_uint64, C.c_uint64, C.c_void_p, u64p,
                                   C.POINTER(Report), u64p, u64p]
        L.inflcut_read.restype = C.c_int
        L.inflcut_bad_loads.restype = C.c_uint64
        _lib = L
    return _lib


class Index:
    """a seek index of the host build; .rc / .report: the build's (rc != OK: there is no index and nothing can be read)"""

    def __init__(self, stream, wrapper, table, spacing=0, group=GROUP_DEFAULT, cut=0, mutant=0, serial=False):
        n = len(table)
        bits = (C.c_uint64 * max(n, 1))(*[t[0] for t in table])
        size = (C.c_uint64 * max(n, 1))(*[t[1] for t in table])
        rc, r = C.c_int(0), Report()
        self.stream = bytes(stream)
        self._h = lib().inflcut_build(mutant, 1 if serial else 0, self.stream, len(self.stream), wrapper, bits, size, n, spacing, group, cut,
                                      C.byref(rc), C.byref(r))
        self.rc, self.report = rc.value, report_dict(r)
        assert (self._h is not None) == (self.rc == OK)

    def close(self):
        if self._h:
            lib().inflcut_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self):
        v = (C.c_uint64 * 6)()
        lib().inflcut_info(self._h, v)
        return dict(zip(("total", "n_entries", "n_points", "cut_bytes", "n_cuts", "surplus"), v))

    def cuts(self):
        n = lib().inflcut_cuts(self._h, None, 0)
        v = (C.c_uint64 * max(3 * n, 1))()
        lib().inflcut_cuts(self._h, v, n)
        return [(v[3 * i], v[3 * i + 1], v[3 * i + 2]) for i in range(n)]

    def set_cut(self, i, cut):
        assert lib().inflcut_set_cut(self._h, i, *cut) == OK

    def read_batch(self, ranges, stream=None, group=GROUP_DEFAULT):
        """ranges: [(off, len)].  stream: what the reads decode from (the build's by default; damaged, but of the same length).
        Returns (rc, [(status rc, got, report dict, the len bytes of the range's buffer, canary intact?)], counts dict, cut counts dict).
        A range's buffer is len bytes of FILL with CANARY bytes of 0xC3 behind it."""
        n = len(ranges)
        stream = self.stream if stream is None else bytes(stream)
        off = (C.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ln = (C.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        at, host = [], bytearray()
        for _off, length in ranges:
            at.append(len(host))
            host += bytes([FILL]) * length + b"\xC3" * CANARY
        buf = C.create_string_buffer(bytes(host), len(host) + 1)
        ata = (C.c_uint64 * max(n, 1))(*at)
        got, reps = (C.c_uint64 * max(n, 1))(), (Report * max(n, 1))()
        counts, cc = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        rc = lib().inflcut_read(self._h, stream, len(stream), off, ln, ata, n, group, C.cast(buf, C.c_void_p), got, reps, counts, cc)
        raw = buf.raw
        res = []
        for k, (_off, length) in enumerate(ranges):
            rep = report_dict(reps[k])
            res.append((E_DATA if reps[k].status else OK, got[k], rep, raw[at[k]:at[k] + length],
                        raw[at[k] + length:at[k] + length + CANARY] == b"\xC3" * CANARY))
        return rc, res, dict(zip(COUNTS, counts)), dict(zip(CUT_COUNTS, cc))

    def read(self, off, length, stream=None, group=GROUP_DEFAULT):
        """one range: (rc, got, report dict, the buffer, canary intact?, counts dict, cut counts dict)"""
        rc, res, counts, cc = self.read_batch([(off, length)], stream, group)
        assert rc == res[0][0]
        return res[0] + (counts, cc)


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, table, spacing, group, cut_bytes, want, ranges, damaged stream or None) -- the file
    inflcut_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"ICC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, table, spacing, group, cut, want, ranges, damaged in cases:
            assert damaged is None or len(damaged) == len(stream)
            f.write(struct.pack("<IQQQQQQQI", wrapper, len(stream), spacing, group, cut, len(table), len(want), len(ranges),
                                1 if damaged is not None else 0))
            for bit, n in table:
                f.write(struct.pack("<QQ", bit, n))
            f.write(bytes(stream))
            if damaged is not None:
                f.write(bytes(damaged))
            f.write(bytes(want))
            for off, length in ranges:
                f.write(struct.pack("<QQ", off, length))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
