"""ctypes binding of tests/inflbig (host build of the large plain members of the members inflate, inflate_bigmembers.h: the call as the
device runs it, discovery and the joint tabled passes lane by lane).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflmembers_binding import CANARY, E_ARG, E_DATA, E_OUT_TOO_SMALL, OK, STATUS, Member, Report, member_tuple, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflbig")
LIB = os.path.join(DIR, "libinflbig.so")
FUZZ = os.path.join(DIR, "inflbig_fuzz")

MUTANT_FILE_POSITION, MUTANT_TRAILER_OFF = 1, 2
STATS = ("parallel", "handed", "spans", "walkers", "entries", "sets")
GROUP_DEFAULT = 256 << 20

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.inflbig_run.argtypes = [C.c_int, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Member),
                                  C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.inflbig_run.restype = C.c_int
        L.inflbig_set.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        L.inflbig_set.restype = C.c_int
        L.inflbig_reset_stats.restype = None
        L.inflbig_stats.argtypes = [C.POINTER(C.c_uint64)]
        L.inflbig_stats.restype = None
        L.inflbig_first_extent.argtypes = [C.c_uint64, C.c_uint64]
        L.inflbig_first_extent.restype = C.c_uint64
        L.inflbig_par_default.restype = C.c_uint64
        L.inflbig_part_size.restype = C.c_uint32
        _lib = L
    return _lib


def run(stream, S, out_cap=0, threshold=1024, index_span=256, group_bytes=GROUP_DEFAULT, mutant=0):
    """the call as the device runs it at member span S and the three settings: (rc, out_len, report dict, member tuples, the bytes of
    the buffer that hold data, canary intact?) like inflmembers_binding.run, and the six counters of the call as a dict"""
    L = lib()
    assert L.inflbig_set(threshold, index_span, group_bytes) == OK
    L.inflbig_reset_stats()
    stream = bytes(stream)
    room = len(stream) // 18 + 2
    buf = C.create_string_buffer(b"\xA5" * out_cap + b"\xC3" * CANARY, out_cap + CANARY) if out_cap else None
    tab = (Member * room)()
    r, got, n = Report(), C.c_uint64(0), C.c_uint64(0)
    rc = L.inflbig_run(mutant, S, stream, len(stream), C.cast(buf, C.c_void_p) if out_cap else None, out_cap, C.byref(got), tab, room, C.byref(n),
                       C.byref(r))
    raw = buf.raw if out_cap else b""
    held = min(got.value, out_cap)
    v = (C.c_uint64 * 6)()
    L.inflbig_stats(v)
    return (rc, got.value, report_dict(r), [member_tuple(tab[k]) for k in range(min(n.value, room))], raw[:held],
            raw[out_cap:] == b"\xC3" * CANARY if out_cap else True), dict(zip(STATS, v))


def first_extent(threshold, S):
    return lib().inflbig_first_extent(threshold, S)


def write_corpus(path, cases):
    """cases: iterable of (file bytes, out_cap, member span, threshold, index span, group bytes) -- the file inflbig_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"IBC1" + struct.pack("<I", len(cases)))
        for stream, cap, S, thr, xs, gb in cases:
            f.write(struct.pack("<QQQQQQ", len(stream), cap, S, thr, xs, gb))
            f.write(bytes(stream))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
