"""ctypes binding of tests/inflmembers (host build of the members inflate, inflate_members.h: the plain serial walk, and the call as
the device runs it with the finder lane by lane or as the plain predicate).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, E_OUT_TOO_SMALL, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflmembers")
LIB = os.path.join(DIR, "libinflmembers.so")
FUZZ = os.path.join(DIR, "inflmembers_fuzz")

NOCAND = (1 << 64) - 1
HINTED = 1
HOW = ["link", "file", "open", "none"]
MUTANT_LAST_CANDIDATE, MUTANT_STOP_GE, MUTANT_TOTAL_IS_BSIZE = 1, 2, 3


class Member(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint64), ("out_off", C.c_uint64), ("out_len", C.c_uint64),
                ("flags", C.c_uint32), ("status", C.c_uint32)]


class Walk(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("n_members", C.c_uint64), ("out_bytes", C.c_uint64),
                ("how", C.c_uint32), ("link", C.c_uint32)]


def member_tuple(m):
    """(in_off, in_len, out_off, out_len, flags, status name)"""
    return m.in_off, m.in_len, m.out_off, m.out_len, m.flags, STATUS[m.status] if m.status < len(STATUS) else m.status


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.inflmembers_serial.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Member), C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.inflmembers_serial.restype = C.c_int
        L.inflmembers_run.argtypes = [C.c_int, C.c_int, C.c_uint64] + L.inflmembers_serial.argtypes + [C.POINTER(C.c_uint64)]
        L.inflmembers_run.restype = C.c_int
        L.inflmembers_scan.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Walk)]
        L.inflmembers_scan.restype = C.c_int
        L.inflmembers_hint.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.inflmembers_hint.restype = C.c_uint32
        L.inflmembers_n_spans.argtypes = [C.c_uint64, C.c_uint64]
        L.inflmembers_set_rooms.argtypes = [C.c_uint64, C.c_uint64]
        L.inflmembers_set_rooms.restype = None
        L.inflmembers_reset_counters.restype = None
        for name in ("n_spans", "chains", "runs", "accepted", "parses", "offsets", "span_min", "span_default"):
            getattr(L, "inflmembers_" + name).restype = C.c_uint64
        L.inflmembers_resumes.restype = C.c_uint32
        L.inflmembers_member_size.restype = C.c_uint32
        _lib = L
    return _lib


def span_default():
    return lib().inflmembers_span_default()


def span_min():
    return lib().inflmembers_span_min()


def n_spans(stream_len, S):
    return lib().inflmembers_n_spans(stream_len, S)


def _call(fn, stream, out_cap, pre, post=()):
    stream = bytes(stream)
    room = len(stream) // 18 + 2
    buf = C.create_string_buffer(b"\xA5" * out_cap + b"\xC3" * CANARY, out_cap + CANARY) if out_cap else None
    tab = (Member * room)()
    r, got, n = Report(), C.c_uint64(0), C.c_uint64(0)
    rc = fn(*pre, stream, len(stream), C.cast(buf, C.c_void_p) if out_cap else None, out_cap, C.byref(got), tab, room, C.byref(n), C.byref(r),
            *post)
    raw = buf.raw if out_cap else b""
    held = min(got.value, out_cap)
    return rc, got.value, report_dict(r), [member_tuple(tab[k]) for k in range(min(n.value, room))], raw[:held], \
        raw[out_cap:] == b"\xC3" * CANARY if out_cap else True


def serial(stream, out_cap=0):
    """the serial walk: (rc, out_len, report dict, member tuples, the bytes of the buffer that hold data, canary intact?).  The buffer
    is out_cap bytes of 0xA5 with CANARY bytes of 0xC3 behind them; out_cap == 0 hands over no buffer (the size query)."""
    return _call(lib().inflmembers_serial, stream, out_cap, ())


def run(stream, S, out_cap=0, lanes=True, mutant=0):
    """the call as the device runs it, at span size S: the same tuple"""
    return _call(lib().inflmembers_run, stream, out_cap, (mutant, 1 if lanes else 0, S), (None,))


def structure(t):
    """a call's result without the HINTED flags: what must equal the serial walk's"""
    rc, n, rep, members, data, canary = t
    return rc, n, rep, [m[:4] + m[5:] for m in members], data, canary


def scan(stream, S, o=0, lanes=True, mutant=0):
    """(candidates, walkers' records as tuples in Walk's field order) of a run that starts at o: one of each per span"""
    stream = bytes(stream)
    n = n_spans(len(stream), S)
    cand = (C.c_uint64 * n)()
    walks = (Walk * n)()
    rc = lib().inflmembers_scan(mutant, 1 if lanes else 0, stream, len(stream), S, o, cand, walks)
    assert rc == OK, rc
    return list(cand), [tuple(getattr(w, f) for f, _t in Walk._fields_) for w in walks]


def hint(stream, o):
    """(is a member hinted at byte o?, does the prefilter let it through?, its claimed extent, its claimed ISIZE)"""
    total, isize = C.c_uint64(0), C.c_uint32(0)
    v = lib().inflmembers_hint(bytes(stream), len(stream), o, C.byref(total), C.byref(isize))
    return bool(v & 1), bool(v & 2), total.value, isize.value


def set_rooms(group=0, room=0):
    """members of one decode turn of Path A and of one launch of Path B; 0: the device's values"""
    lib().inflmembers_set_rooms(group, room)


def counters():
    L = lib()
    return dict(chains=L.inflmembers_chains(), runs=L.inflmembers_runs(), accepted=L.inflmembers_accepted(), parses=L.inflmembers_parses(),
                offsets=L.inflmembers_offsets())


def reset_counters():
    lib().inflmembers_reset_counters()


def write_corpus(path, cases):
    """cases: iterable of (file bytes, span_bytes, out_cap) -- the file inflmembers_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"IMC1" + struct.pack("<I", len(cases)))
        for stream, S, cap in cases:
            f.write(struct.pack("<QQQ", len(stream), cap, S))
            f.write(bytes(stream))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
