"""ctypes binding of tests/inflindex (host build of the inflate index, inflate_index.h: the finder lane by lane and as the plain
predicate, the walkers, the link, and the combined call judged by the three-pass tabled host build).  TEST INFRASTRUCTURE."""
import ctypes as C
import os
import struct
import subprocess

from inflwrite_binding import CANARY, E_ARG, E_DATA, E_OUT_TOO_SMALL, OK, STATUS, Report, report_dict  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "inflindex")
LIB = os.path.join(DIR, "libinflindex.so")
FUZZ = os.path.join(DIR, "inflindex_fuzz")

NOCAND = (1 << 64) - 1
HOW = ["link", "final", "failed", "none"]
GROUP_DEFAULT = 256 << 20
MUTANT_STOP_GE, MUTANT_LINK_CANDIDATE, MUTANT_BFINAL = 1, 2, 3


class Walk(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end_bit", C.c_uint64), ("count", C.c_uint64), ("how", C.c_uint32), ("link", C.c_uint32),
                ("btype", C.c_uint32), ("status", C.c_uint32), ("n_stored", C.c_uint32), ("n_fixed", C.c_uint32),
                ("n_dynamic", C.c_uint32), ("reserved", C.c_uint32), ("n_blocks", C.c_uint64), ("bit", C.c_uint64),
                ("in_pos", C.c_uint64)]


class BlockInfo(C.Structure):
    _fields_ = [("btype", C.c_uint32), ("bfinal", C.c_uint32), ("n_tokens", C.c_uint32), ("reserved", C.c_uint32),
                ("in_bytes", C.c_uint64), ("bit_start", C.c_uint64)]


def walk_tuple(w):
    return tuple(getattr(w, f) for f, _t in Walk._fields_)


def block_dict(b):
    return {f: getattr(b, f) for f, _t in BlockInfo._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", DIR, "-s"])
        L = C.CDLL(LIB)
        L.inflindex_n_spans.argtypes = [C.c_uint64, C.c_uint64]
        L.inflindex_n_spans.restype = C.c_uint64
        L.inflindex_scan.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Walk)]
        L.inflindex_scan.restype = C.c_int
        L.inflindex_index.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(BlockInfo), C.POINTER(C.c_uint64),
                                      C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.inflindex_index.restype = C.c_int
        L.inflindex_parallel.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(Report)]
        L.inflindex_parallel.restype = C.c_int
        L.inflindex_blocks.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint64]
        L.inflindex_blocks.restype = C.c_uint64
        L.inflindex_is_start.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_uint64]
        L.inflindex_is_start.restype = C.c_uint32
        for name in ("parses", "offsets", "span_min", "span_default"):
            getattr(L, "inflindex_" + name).restype = C.c_uint64
        L.inflindex_walk_size.restype = C.c_uint32
        L.inflindex_reset_counters.restype = None
        _lib = L
    return _lib


def span_default():
    return lib().inflindex_span_default()


def n_spans(stream_len, S):
    return lib().inflindex_n_spans(stream_len, S)


def scan(stream, wrapper, S, lanes=True, mutant=0):
    """(candidates, walkers' records as tuples in Walk's field order): one of each per span"""
    n = n_spans(len(stream), S)
    cand = (C.c_uint64 * n)()
    recs = (Walk * n)()
    rc = lib().inflindex_scan(mutant, 1 if lanes else 0, bytes(stream), len(stream), wrapper, S, cand, recs)
    assert rc == OK, rc
    return list(cand), [walk_tuple(w) for w in recs]


def index(stream, wrapper, S, cap=None, mutant=0):
    """(rc, n_blocks, table as a list of dicts, the span of every entry's walker, report dict); cap None: room for every span"""
    room = n_spans(len(stream), S) if cap is None else cap
    blocks = (BlockInfo * max(room, 1))()
    spans = (C.c_uint64 * max(room, 1))()
    n = C.c_uint64(0)
    r = Report()
    rc = lib().inflindex_index(mutant, bytes(stream), len(stream), wrapper, S, blocks if room else None, spans if room else None, room,
                               C.byref(n), C.byref(r))
    k = n.value if rc in (OK, E_DATA) else 0
    return rc, n.value, [block_dict(blocks[i]) for i in range(k)], [spans[i] for i in range(k)], report_dict(r)


def parallel(stream, wrapper, S, out_cap=0, group=GROUP_DEFAULT, mutant=0):
    """Returns (rc, out_len, report dict, the out_cap bytes of the buffer, canary intact?) like inflwrite_binding.inflate"""
    buf = C.create_string_buffer(b"\xA5" * out_cap + b"\xC3" * CANARY, out_cap + CANARY) if out_cap else None
    r = Report()
    got = C.c_uint64(0)
    rc = lib().inflindex_parallel(mutant, bytes(stream), len(stream), wrapper, S, group, C.cast(buf, C.c_void_p) if out_cap else None,
                                  out_cap, C.byref(got), C.byref(r))
    raw = buf.raw if out_cap else b""
    return rc, got.value, report_dict(r), raw[:out_cap], raw[out_cap:] == b"\xC3" * CANARY if out_cap else True


def blocks(stream, wrapper=0):
    """[(bit, BFINAL | BTYPE << 1)] of every block of the stream's serial walk that decodes (a failing block ends the list)"""
    cap = 8 * len(stream) // 3 + 1
    bits = (C.c_uint64 * cap)()
    heads = (C.c_uint32 * cap)()
    n = lib().inflindex_blocks(bytes(stream), len(stream), wrapper, bits, heads, cap)
    return [(bits[k], heads[k]) for k in range(n)]


def is_start(stream, wrapper, bit):
    """(does the predicate hold at this raw-deflate bit offset?, does the prefilter let it through?)"""
    v = lib().inflindex_is_start(bytes(stream), len(stream), wrapper, bit)
    return bool(v & 1), bool(v & 2)


def counters():
    return dict(parses=lib().inflindex_parses(), offsets=lib().inflindex_offsets())


def reset_counters():
    lib().inflindex_reset_counters()


def write_corpus(path, cases):
    """cases: iterable of (stream, wrapper, out_cap, span_bytes, group_bytes) -- the file inflindex_fuzz reads"""
    cases = list(cases)
    with open(path, "wb") as f:
        f.write(b"IXC1" + struct.pack("<I", len(cases)))
        for stream, wrapper, cap, S, group in cases:
            f.write(struct.pack("<IQQQQ", wrapper, len(stream), cap, S, group))
            f.write(bytes(stream))


def run_fuzz(path):
    """the sanitizer program over a corpus file: (exit status, output)"""
    lib()
    p = subprocess.run([FUZZ, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    return p.returncode, p.stdout
