"""ctypes binding of tests/inflseek (host build of the seek points, inflate_seek.h: the build with its kept windows, a read as its plan
and the three passes, and the two mutants).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflseek")
LIB = os.path.join(DIR, "libinflseek.so")
FUZZ = os.path.join(DIR, "inflseek_fuzz")

GROUP_DEFAULT = 256 << 20  # MI355_CFG_INFLATE_GROUP_BYTES's default
GROUP_MIN = 64 << 10       # ... and its minimum
MUTANT_POINTS, MUTANT_RESOLVE = 1, 2
FILL = 0xA5
COUNTS = ("entries", "symbols", "steps", "sets")

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        u64p = C.POINTER(C.c_uint64)
        L.inflseek_build.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int, u64p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int),
                                     C.POINTER(Report)]
        L.inflseek_build.restype = C.c_void_p
        L.inflseek_free.argtypes = [C.c_void_p]
        L.inflseek_free.restype = None
        L.inflseek_info.argtypes = [C.c_void_p, u64p]
        L.inflseek_info.restype = None
        L.inflseek_points.argtypes = [C.c_void_p, u64p, C.c_uint64]
        L.inflseek_points.restype = C.c_uint64
        L.inflseek_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, u64p, u64p, u64p, C.c_uint64, C.c_uint64, C.c_void_p, u64p,
                                    C.POINTER(Report), u64p, u64p]
        L.inflseek_read.restype = C.c_int
        L.inflseek_unfenced_loads.restype = C.c_uint64
        L.inflseek_part_size.restype = C.c_uint32
        _lib = L
    return _lib


class Index:
    """a seek index of the host build; .rc / .report: the build's (rc != OK: there is no index and nothing can be read)"""

    def __init__(self, stream, wrapper, table, spacing=0, group=GROUP_DEFAULT, mutant=0):
        n = len(table)
        bits = (C.c_uint64 * max(n, 1))(*[t[0] for t in table])
        size = (C.c_uint64 * max(n, 1))(*[t[1] for t in table])
        rc, r = C.c_int(0), Report()
        self.stream = bytes(stream)
        self._h = lib().inflseek_build(mutant, self.stream, len(self.stream), wrapper, bits, size, n, spacing, group, C.byref(rc), C.byref(r))
        self.rc, self.report = rc.value, report_dict(r)
        assert (self._h is not None) == (self.rc == OK)

    def close(self):
        if self._h:
            lib().inflseek_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self):
        v = (C.c_uint64 * 7)()
        lib().inflseek_info(self._h, v)
        return dict(zip(("total", "n_entries", "n_points", "spacing", "device_bytes", "stream_len", "wrapper"), v))

    def points(self):
        n = lib().inflseek_points(self._h, None, 0)
        v = (C.c_uint64 * max(2 * n, 1))()
        lib().inflseek_points(self._h, v, n)
        return [(v[2 * i], v[2 * i + 1]) for i in range(n)]

    def read_batch(self, ranges, stream=None, group=GROUP_DEFAULT, aligns=None):
        """ranges: [(off, len)].  stream: what the reads decode from (the build's by default; damaged, but of the same length).
        aligns: per range, the class mod 8 of its buffer's address (None: back to back as they come).
        Returns (rc, [(status rc, got, report dict, the len bytes of the range's buffer, canary intact?)], counts dict, stray stores).
        A range's buffer is len bytes of FILL with CANARY bytes of 0xC3 behind it."""
        n = len(ranges)
        stream = self.stream if stream is None else bytes(stream)
        off = (C.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ln = (C.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        at, host = [], bytearray()
        for k, (_off, length) in enumerate(ranges):
            if aligns is not None:
                host += bytes(-len(host) % 8 + aligns[k])
            at.append(len(host))
            host += bytes([FILL]) * length + b"\xC3" * CANARY
        buf = C.create_string_buffer(bytes(host), len(host) + 1)
        assert C.addressof(buf) % 8 == 0
        ata = (C.c_uint64 * max(n, 1))(*at)
        got, reps = (C.c_uint64 * max(n, 1))(), (Report * max(n, 1))()
        counts, stray = (C.c_uint64 * 4)(), C.c_uint64(0)
        rc = lib().inflseek_read(self._h, stream, len(stream), off, ln, ata, n, group, C.cast(buf, C.c_void_p), got, reps, counts, C.byref(stray))
        raw = buf.raw
        res = []
        for k, (_off, length) in enumerate(ranges):
            rep = report_dict(reps[k])
            res.append((E_DATA if reps[k].status else OK, got[k], rep, raw[at[k]:at[k] + length],
                        raw[at[k] + length:at[k] + length + CANARY] == b"\xC3" * CANARY))
        return rc, res, dict(zip(COUNTS, counts)), stray.value

    def read(self, off, length, stream=None, group=GROUP_DEFAULT):
        """one range: (rc, got, report dict, the buffer, canary intact?, counts dict, stray stores)"""
        rc, res, counts, stray = self.read_batch([(off, length)], stream, group)
        assert rc == res[0][0]
        return res[0] + (counts, stray)


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, table, spacing, group, want, ranges, damaged stream or None) -- the file inflseek_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"ISC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, table, spacing, group, want, ranges, damaged in cases:
            assert damaged is None or len(damaged) == len(stream)
            f.write(struct.pack("<IQQQQQQI", wrapper, len(stream), spacing, group, len(table), len(want), len(ranges), 1 if damaged is not None else 0))
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
