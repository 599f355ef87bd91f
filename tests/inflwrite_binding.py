"""ctypes binding of tests/inflwrite (host build of the inflate decisions, inflate_write.h).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflwrite")
LIB = os.path.join(DIR, "libinflwrite.so")
FUZZ = os.path.join(DIR, "inflwrite_fuzz")

STATUS = ["OK", "FRAME", "BTYPE", "STORED", "LENGTHS", "CODE", "DISTANCE", "MISMATCH", "LENGTH", "TABLE", "TRUNCATED", "TRAILER",
          "CHECKSUM"]
INFLATE_STATUS = [s for s in STATUS if s not in ("MISMATCH", "LENGTH", "TABLE")]  # what an inflate can report
OK, E_ARG, E_OUT_TOO_SMALL, E_DATA = 0, -1, -2, -8
CANARY = 64


class Report(C.Structure):
    _fields_ = [("status", C.c_uint32), ("reserved", C.c_uint32), ("bit", C.c_uint64), ("out_pos", C.c_uint64), ("out_len", C.c_uint64),
                ("n_blocks", C.c_uint64), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32), ("n_dynamic", C.c_uint32),
                ("ms", C.c_float)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.inflwrite_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.inflwrite_inflate.restype = C.c_int
        L.inflwrite_inflate_lanes.argtypes = L.inflwrite_inflate.argtypes
        L.inflwrite_inflate_lanes.restype = C.c_int
        L.inflwrite_unfenced_loads.restype = C.c_uint64
        L.inflwrite_fences.restype = C.c_uint64
        L.inflwrite_report_size.restype = C.c_uint32
        L.inflwrite_rec_size.restype = C.c_uint32
        _lib = L
    return _lib


def report_dict(r):
    return dict(status=STATUS[r.status] if r.status < len(STATUS) else r.status, bit=r.bit, out_pos=r.out_pos, out_len=r.out_len,
                n_blocks=r.n_blocks, n_stored=r.n_stored, n_fixed=r.n_fixed, n_dynamic=r.n_dynamic)


def inflate(stream, wrapper=0, out_cap=0, lanes=False):
    """Returns (rc, out_len, report dict, the out_cap bytes of the buffer, canary intact?).  The buffer is out_cap bytes filled with
    0xA5 and CANARY bytes of 0xC3 behind them; out_cap == 0 hands the decoder a NULL buffer (the size query)."""
    buf = C.create_string_buffer(b"\xA5" * out_cap + b"\xC3" * CANARY, out_cap + CANARY) if out_cap else None
    r = Report()
    n = C.c_uint64(0)
    fn = lib().inflwrite_inflate_lanes if lanes else lib().inflwrite_inflate
    rc = fn(bytes(stream), len(stream), wrapper, C.cast(buf, C.c_void_p) if out_cap else None, out_cap, C.byref(n), C.byref(r))
    raw = buf.raw if out_cap else b""
    return rc, n.value, report_dict(r), raw[:out_cap], raw[out_cap:] == b"\xC3" * CANARY if out_cap else True


def cap_for(stream, wrapper, want):
    """the buffer size a test gives a case: zlib's length for an accepted one; for a rejected one the exact size if the stream is
    structurally valid (so that its checksum is judged), else 20 000 bytes (some stop short of it, some run past)"""
    if want is not None:
        return len(want)
    rc, n, _rep, _buf, _ok = inflate(stream, wrapper, 0)
    return n if rc == E_OUT_TOO_SMALL else 20000


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, out_cap) -- the file inflwrite_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"IWC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, cap in cases:
            f.write(struct.pack("<IQQ", wrapper, len(stream), cap))
            f.write(bytes(stream))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
