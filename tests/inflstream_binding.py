"""ctypes binding of tests/inflstream (host build of the stream-inflate decisions, inflate_stream.h, with a model of the handle).
TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, E_OUT_TOO_SMALL, OK, STATUS, Report

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflstream")
LIB = os.path.join(DIR, "libinflstream.so")
FUZZ = os.path.join(DIR, "inflstream_fuzz")
E_STATE = -6
FP_NEED_MORE, FP_BAD, FP_OK = 0, 1, 2
MUTANTS = {"history_not_shifted": 1, "seam_off_by_one": 2, "commit_inside_block": 3, "truncated_is_final": 4, "dist_this_write_only": 5}


class State(C.Structure):
    _fields_ = [("total_in", C.c_uint64), ("total_out", C.c_uint64), ("pending_in", C.c_uint64), ("need_out", C.c_uint64),
                ("done", C.c_uint32), ("failed", C.c_uint32), ("adler_or_crc", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.ism_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int]
        L.ism_new.restype = C.c_void_p
        L.ism_write.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.ism_write.restype = C.c_int
        L.ism_finish.argtypes = [C.c_void_p, C.POINTER(Report)]
        L.ism_finish.restype = C.c_int
        L.ism_state.argtypes = [C.c_void_p, C.POINTER(State)]
        L.ism_state.restype = None
        L.ism_reset.argtypes = [C.c_void_p]
        L.ism_reset.restype = None
        L.ism_free.argtypes = [C.c_void_p]
        L.ism_free.restype = None
        L.ism_set_mutant.argtypes = [C.c_int]
        L.ism_set_mutant.restype = None
        L.ism_unfenced_loads.restype = C.c_uint64
        L.ism_frame_prefix.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.ism_frame_prefix.restype = C.c_uint32
        L.ism_block_ends.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64]
        L.ism_block_ends.restype = C.c_uint64
        _lib = L
    return _lib


def report_dict(r):
    return dict(status=STATUS[r.status] if r.status < len(STATUS) else r.status, bit=r.bit, out_pos=r.out_pos, out_len=r.out_len)


def state_dict(s):
    return dict(total_in=s.total_in, total_out=s.total_out, pending_in=s.pending_in, need_out=s.need_out, done=s.done,
                failed=STATUS[s.failed] if s.failed < len(STATUS) else s.failed, adler_or_crc=s.adler_or_crc)


class Model:
    """The handle model; the same methods as DeviceHandle of tests/test_inflate_stream_gpu.py, so one driver serves both."""

    def __init__(self, wrapper=0, zdict=None, lanes=False):
        self.h = lib().ism_new(wrapper, zdict, len(zdict) if zdict else 0, 1 if lanes else 0)
        assert self.h, "ism_new refused its arguments"

    def write(self, chunk, cap):
        """(rc, the bytes handed over, report dict, canary intact?)"""
        buf = C.create_string_buffer(b"\xA5" * cap + b"\xC3" * CANARY, cap + CANARY) if cap else None
        r = Report()
        n = C.c_uint64(0)
        rc = lib().ism_write(self.h, bytes(chunk) if chunk else None, len(chunk), C.cast(buf, C.c_void_p) if cap else None, cap, C.byref(n),
                             C.byref(r))
        raw = buf.raw if cap else b""
        assert n.value <= cap
        return rc, raw[:n.value], report_dict(r), raw[cap:] == b"\xC3" * CANARY if cap else True

    def finish(self):
        r = Report()
        rc = lib().ism_finish(self.h, C.byref(r))
        return rc, report_dict(r)

    def state(self):
        s = State()
        lib().ism_state(self.h, C.byref(s))
        return state_dict(s)

    def reset(self):
        lib().ism_reset(self.h)

    def close(self):
        if self.h:
            lib().ism_free(self.h)
            self.h = None

    __del__ = close


def frame_prefix(s, wrapper):
    n = C.c_uint64(0)
    r = lib().ism_frame_prefix(bytes(s), len(s), wrapper, C.byref(n))
    return r, n.value


def block_ends(stream, wrapper, out_total, zdict=None):
    """[(k, out_pos)]: the prefix lengths at which one more block counts as complete (the BFINAL block: with its trailer), and the
    bytes in front of that block end"""
    cap = len(stream) + 1
    arr = (C.c_uint64 * (2 * cap))()
    n = lib().ism_block_ends(bytes(stream), len(stream), wrapper, zdict, len(zdict) if zdict else 0, out_total, arr, cap)
    return [(arr[2 * i], arr[2 * i + 1]) for i in range(min(n, cap))]


def set_mutant(name):
    lib().ism_set_mutant(MUTANTS[name] if name else 0)


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, zdict or None, [(piece length, cap)]) -- the file inflstream_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"ISC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, zdict, pieces in cases:
            zdict = zdict or b""
            assert sum(n for n, _ in pieces) == len(stream)
            f.write(struct.pack("<IIQQ", wrapper, len(pieces), len(stream), len(zdict)))
            f.write(bytes(stream) + bytes(zdict))
            for n, cap in pieces:
                f.write(struct.pack("<QQ", n, cap))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
