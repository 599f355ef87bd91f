"""ctypes binding of tests/bgzfread (host build of the BGZF reads, bgzf_read.h: the index from a table or from the file's own claims,
virtual offsets, a read as its plan with the members decoded and clipped lane by lane, and the three mutants).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import E_ARG, E_DATA, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "bgzfread")
LIB = os.path.join(DIR, "libbgzfread.so")
FUZZ = os.path.join(DIR, "bgzfread_fuzz")

E_OUT_TOO_SMALL, E_UNSUPPORTED = -2, -4
GROUP_DEFAULT = 256 << 20  # MI355_CFG_INFLATE_GROUP_BYTES's default
GROUP_MIN = 64 << 10       # ... and its minimum
SPAN_DEFAULT = 65536
MUTANT_SHARING, MUTANT_SEAM, MUTANT_LENGTH = 1, 2, 3
FILL = 0xA5
GUARD = 64
ROOM_MAX = 1 << 22
COUNTS = ("distinct", "in_place", "scratch", "pieces", "sets")

_lib = None


class Member(C.Structure):
    """mi355_member_info"""
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint64), ("out_off", C.c_uint64), ("out_len", C.c_uint64),
                ("flags", C.c_uint32), ("status", C.c_uint32)]


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        u64p = C.POINTER(C.c_uint64)
        L.bgzfread_build.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.POINTER(Report)]
        L.bgzfread_build.restype = C.c_void_p
        L.bgzfread_from_members.argtypes = [C.POINTER(Member), C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]
        L.bgzfread_from_members.restype = C.c_void_p
        L.bgzfread_free.argtypes = [C.c_void_p]
        L.bgzfread_free.restype = None
        L.bgzfread_info.argtypes = [C.c_void_p, u64p]
        L.bgzfread_info.restype = None
        L.bgzfread_members.argtypes = [C.c_void_p, C.POINTER(Member), C.c_uint64]
        L.bgzfread_members.restype = C.c_uint64
        L.bgzfread_voffset.argtypes = [C.c_void_p, C.c_uint64, u64p]
        L.bgzfread_uoffset.argtypes = [C.c_void_p, C.c_uint64, u64p]
        L.bgzfread_read.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint64, u64p, u64p, u64p, C.c_uint64, C.c_uint64, C.c_void_p, u64p,
                                    C.POINTER(C.c_int32), C.POINTER(Report), u64p]
        L.bgzfread_read.restype = C.c_int
        L.bgzfread_unfenced_loads.restype = C.c_uint64
        L.bgzfread_piece_size.restype = C.c_uint32
        L.bgzfread_set_members.restype = C.c_uint32
        _lib = L
    return _lib


def member_rows(members):
    """[dict or tuple (in_off, in_len, out_off, out_len[, flags[, status]])] -> a ctypes array of mi355_member_info"""
    arr = (Member * max(len(members), 1))()
    for k, m in enumerate(members):
        if isinstance(m, dict):
            st = m.get("status", 0)
            m = (m["in_off"], m["in_len"], m["out_off"], m["out_len"], m.get("flags", 0), STATUS.index(st) if isinstance(st, str) else st)
        m = tuple(m) + (0, 0)[len(m) - 4:]
        arr[k].in_off, arr[k].in_len, arr[k].out_off, arr[k].out_len, arr[k].flags, arr[k].status = m
    return arr


def layout(lengths, aligns=None):
    """the arena of a batch of buffers: (offsets, bytes) -- every buffer is GUARD bytes of 0xC3, len bytes of FILL, GUARD bytes of 0xC3;
    aligns: per buffer, the class mod 16 of its first byte's address in a 16-byte aligned arena"""
    at, host = [], bytearray()
    for k, n in enumerate(lengths):
        host += b"\xC3" * GUARD
        if aligns is not None:
            host += b"\xC3" * ((aligns[k] - len(host)) % 16)
        at.append(len(host))
        host += bytes([FILL]) * n + b"\xC3" * GUARD
    return at, bytes(host)


def guards_intact(raw, at, n):
    g = b"\xC3" * GUARD
    return raw[at - GUARD:at] == g and raw[at + n:at + n + GUARD] == g


class Index:
    """a BGZF index of the host build.  Index(file=...) builds it from the file's own claims, Index(members=..., file_len=...) from
    a table; .rc / .report: the build's (rc != OK: there is no index)"""

    def __init__(self, file=None, members=None, file_len=None, span=SPAN_DEFAULT):
        rc, r = C.c_int(0), Report()
        self.file = None if file is None else bytes(file)
        if members is not None:
            self._h = lib().bgzfread_from_members(member_rows(members) if len(members) else None, len(members), file_len, C.byref(rc))
            self.report = None
        else:
            self._h = lib().bgzfread_build(self.file, len(self.file), span, C.byref(rc), C.byref(r))
            self.report = report_dict(r)
        self.rc = rc.value
        assert (self._h is not None) == (self.rc == OK)

    def close(self):
        if self._h:
            lib().bgzfread_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self):
        v = (C.c_uint64 * 4)()
        lib().bgzfread_info(self._h, v)
        return dict(zip(("total", "n_members", "file_len", "max_out_len"), v))

    def members(self):
        n = lib().bgzfread_members(self._h, None, 0)
        arr = (Member * max(n, 1))()
        lib().bgzfread_members(self._h, arr, n)
        return [dict(in_off=m.in_off, in_len=m.in_len, out_off=m.out_off, out_len=m.out_len, flags=m.flags, status=STATUS[m.status])
                for m in arr[:n]]

    def voffset(self, u):
        v = C.c_uint64(0)
        rc = lib().bgzfread_voffset(self._h, u, C.byref(v))
        return rc, v.value

    def uoffset(self, v):
        u = C.c_uint64(0)
        rc = lib().bgzfread_uoffset(self._h, v, C.byref(u))
        return rc, u.value

    def read_batch(self, ranges, file=None, budget=GROUP_DEFAULT, aligns=None, mutant=0):
        """ranges: [(off, len)].  file: what the reads decode from (the build's by default; damaged, but of the same length).
        Returns (rc, [(status, got, report dict, the len bytes of the range's buffer, guards intact?)], counts dict)."""
        n = len(ranges)
        file = self.file if file is None else bytes(file)
        off = (C.c_uint64 * max(n, 1))(*[r[0] for r in ranges])
        ln = (C.c_uint64 * max(n, 1))(*[r[1] for r in ranges])
        rooms = [min(r[1], ROOM_MAX) for r in ranges]  # (a range far beyond the end of the file gets no more room than this)
        at, host = layout(rooms, aligns)
        buf = (C.c_uint8 * (len(host) + 32))()
        pad = -C.addressof(buf) % 16
        C.memmove(C.addressof(buf) + pad, host, len(host))
        ata = (C.c_uint64 * max(n, 1))(*at)
        got, st, reps = (C.c_uint64 * max(n, 1))(), (C.c_int32 * max(n, 1))(), (Report * max(n, 1))()
        counts = (C.c_uint64 * 5)()
        rc = lib().bgzfread_read(self._h, mutant, file, len(file), off, ln, ata, n, budget, C.c_void_p(C.addressof(buf) + pad), got, st, reps, counts)
        raw = bytes(buf)[pad:pad + len(host)]
        res = [(st[k], got[k], report_dict(reps[k]), raw[at[k]:at[k] + length], guards_intact(raw, at[k], length)) for k, length in enumerate(rooms)]
        return rc, res, dict(zip(COUNTS, counts))

    def read(self, off, length, file=None, budget=GROUP_DEFAULT, align=0, mutant=0):
        """one range: (rc, got, report dict, the buffer, guards intact?, counts dict)"""
        rc, res, counts = self.read_batch([(off, length)], file, budget, [align], mutant)
        assert rc == res[0][0]
        return res[0] + (counts,)


def write_corpus(path, cases):
    """cases: iterable of (file, damaged file or None, budget, want, ranges) -- the file bgzfread_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"BRC1" + struct.pack("<I", len(cases)))
        for file, damaged, budget, want, ranges in cases:
            assert damaged is None or len(damaged) == len(file)
            f.write(struct.pack("<QQQQI", len(file), budget, len(want), len(ranges), 1 if damaged is not None else 0))
            f.write(bytes(file))
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
