"""Cases for the inflate entry points (include/mi355_deflate.h mi355_inflate*): seeded, shared by the CPU test of the host build
(test_inflate_cases.py) and the GPU test (test_inflate_gpu.py).  TEST INFRASTRUCTURE.

  (a) every stream of verify_cases.streams(), mutations() and hand()
  (b) write_path()  fixed-code blocks assembled bit by bit that force the edges of the write path: matches whose source lies in the
                    literals just gathered or in what the previous match step wrote, periods that do not divide 64, matches
                    reaching into stored pieces of every alignment class, the largest distance, several blocks in a row
  (c) framed()      hand-built frames for the statuses the imported groups may lack: FRAME, TRAILER and CHECKSUM of both wrappers

A case is Case(name, stream, wrapper, label, want): label = the status name verify_cases.hand() gives it (or None), want = the
bytes zlib inflates the stream to, or None when zlib refuses it.  The judge is zlib alone: accepted means no zlib.error, the end
of the stream reached and nothing left over; the expected bytes are zlib's output, not the `input` the verify case carries.
"""
import collections
import functools
import random
import struct
import zlib

import verify_cases as vc
from verify_cases import WBITS, BitWriter, dyn_block, fixed_ll, gzip_frame

Case = collections.namedtuple("Case", "name stream wrapper label want group")


def zlib_inflates(stream, wrapper):
    """the bytes zlib inflates `stream` to, or None if it refuses it, does not reach its end or leaves bytes over"""
    d = zlib.decompressobj(WBITS[wrapper])
    try:
        out = d.decompress(bytes(stream)) + d.flush()
    except zlib.error:
        return None
    return out if d.eof and d.unused_data == b"" else None


# ---- (b): matches and stored pieces in fixed-code blocks ---------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]


def put_match(w, length, dist):
    """a (length, distance) pair in the fixed code (RFC 1951 3.2.5, 3.2.6)"""
    lc = max(k for k in range(29) if LEN_BASE[k] <= length)
    fixed_ll(w, 257 + lc).put(length - LEN_BASE[lc], LEN_EXTRA[lc])
    dc = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return w.code(dc, 5).put(dist - DIST_BASE[dc], DIST_EXTRA[dc])


def put_lits(w, data):
    for c in data:
        fixed_ll(w, c)
    return w


def fixed_open(w, bfinal):
    return w.put(bfinal, 1).put(1, 2)


def stored(w, data, bfinal=0):
    return w.put(bfinal, 1).put(0, 2).align().put(len(data), 16).put(~len(data) & 0xFFFF, 16).raw(data)


DISTS = (1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 66, 70)
LENS = (3, 4, 63, 64, 65, 128, 129, 258)
SEED70 = bytes(range(33, 103))  # 70 distinct bytes
STORED_SIZES = (0, 1, 7, 8, 511, 512, 513, 65535)


@functools.lru_cache(maxsize=None)
def write_path():
    """[(name, stream)]: raw streams, every one valid"""
    out = []
    rnd = random.Random(20250118)
    # a seed of 70 distinct bytes, then every length at one distance, each match preceded by 0, 1 or 64 fresh literals: with 64 the
    # source of a short distance lies inside the literals just gathered, with 0 in what the previous match's last step wrote
    for dist in DISTS:
        for nlit in (0, 1, 64):
            w = put_lits(fixed_open(BitWriter(), 1), SEED70)
            for length in LENS:
                put_lits(w, bytes(rnd.getrandbits(8) for _ in range(nlit)))
                put_match(w, length, dist)
            out.append(("match_d%d_lit%d" % (dist, nlit), fixed_ll(w, 256).bytes()))
    # a stored piece behind 9 literals (its destination starts at an odd address whatever the buffer's), then a match reaching into
    # its tail and one that copies from the stream's start through it
    for n in STORED_SIZES:
        piece = bytes(rnd.getrandbits(8) for _ in range(n))
        w = fixed_ll(put_lits(fixed_open(BitWriter(), 0), SEED70[:9]), 256)
        stored(w, piece)
        fixed_open(w, 1)
        put_match(w, 20, min(n, 300) + 3)
        put_match(w, 258, min(n + 9 + 20, 32768))
        out.append(("stored_%d_then_match" % n, fixed_ll(w, 256).bytes()))
    # the largest distance at the first position that allows it, the longest length
    big = bytes(rnd.getrandbits(8) for _ in range(32768))
    w = stored(BitWriter(), big[:32767])
    stored(w, big[32767:])
    fixed_open(w, 1)
    put_match(w, 258, 32768)
    put_match(w, 258, 32768)
    out.append(("distance_32768_at_32768_len_258", fixed_ll(w, 256).bytes()))
    # three consecutive fixed blocks, a match of the third reaching into the first
    w = fixed_ll(put_lits(fixed_open(BitWriter(), 0), b"first block, "), 256)
    fixed_ll(put_match(put_lits(fixed_open(w, 0), b"second, "), 5, 8), 256)
    fixed_ll(put_match(put_lits(fixed_open(w, 1), b"third: "), 13, 33), 256)
    out.append(("three_fixed_blocks", w.bytes()))
    # a dynamic block after a stored one (the stored piece ends on a byte, the dynamic block begins there)
    A = ord("a")
    out.append(("dynamic_after_stored", stored(BitWriter(), b"xyz").bytes() +
                dyn_block({A: 1, 256: 2, 257: 2}, {0: 1}, [A, A, A, 257, ("d", 0), 256])))
    return out


# ---- (c): frames ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def framed():
    """[(name, stream, wrapper)]"""
    data = vc.pg11()[:3000]
    raw = zlib.compress(data, 6)[2:-4]
    z = zlib.compress(data, 6)
    g = gzip_frame(raw, data, vc.GZ_HEADERS["name"])
    out = [("zlib_ok", z, 1), ("gzip_ok", g, 2)]
    out.append(("zlib_fdict", bytes([0x78, 0xBB]) + z[2:], 1))  # FDICT set, FCHECK right
    out.append(("zlib_cm_7", bytes([0x77, 0x9C]) + z[2:], 1))
    out.append(("zlib_5_bytes", z[:5], 1))
    out.append(("gzip_magic", b"\x1f\x8c" + g[2:], 2))
    out.append(("gzip_reserved_flag", g[:3] + bytes([g[3] | 0x80]) + g[4:], 2))
    out.append(("gzip_17_bytes", g[:17], 2))
    out.append(("gzip_name_without_end", g[:10] + b"x" * (len(g) - 10), 2))
    out.append(("raw_byte_behind", raw + b"\0", 0))
    out.append(("zlib_byte_behind", z + b"\0", 1))
    out.append(("gzip_byte_behind", g + b"\0", 2))
    out.append(("gzip_second_member", g + g, 2))
    out.append(("zlib_adler_low", z[:-1] + bytes([z[-1] ^ 1]), 1))
    out.append(("zlib_adler_high", z[:-4] + bytes([z[-4] ^ 0x80]) + z[-3:], 1))
    out.append(("gzip_crc", g[:-8] + bytes([g[-8] ^ 1]) + g[-7:], 2))
    out.append(("gzip_isize", g[:-1] + bytes([g[-1] ^ 1]), 2))
    out.append(("gzip_empty", gzip_frame(zlib.compress(b"", 6)[2:-4], b"", vc.GZ_HEADERS["blank"]), 2))
    out.append(("zlib_empty", zlib.compress(b"", 6), 1))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """every Case of the three groups, judged by zlib"""
    out = []

    def add(group, name, stream, wrapper, label=None):
        out.append(Case(group + ":" + name, bytes(stream), wrapper, label, zlib_inflates(stream, wrapper), group))

    for name, s, _d, w, _tab in vc.streams():
        add("streams", name, s, w)
    for name, s, _d, w in vc.mutations():
        add("mutations", name, s, w)
    for name, s, _d, w, status in vc.hand():
        add("hand", name, s, w, status)
    for name, s in write_path():
        add("write_path", name, s, 0)
    for name, s, w in framed():
        add("framed", name, s, w)
    return out


def accepted():
    return [c for c in corpus() if c.want is not None]


def rejected():
    return [c for c in corpus() if c.want is None]
