"""Cases for the verify entry points (include/mi355_deflate.h mi355_deflate_verify*): seeded, shared by the CPU test of the host
build (test_verify_cases.py) and the GPU test (test_verify_gpu.py).  TEST INFRASTRUCTURE.

  (a) streams()    valid streams from the oracle and from Python's zlib over inputs that reach every path of the decoder
  (b) mutations()  bit flips, truncations, appended bytes and trailer edits of a raw and a zlib stream
  (c) hand()       streams assembled bit by bit, each with the status it must give
  (d) edits()      a valid stream against an input with one byte changed

A case is (name, stream, input, wrapper[, table]).  The judge of (b) and (c) is zlib_accepts().
"""
import functools
import glob
import os
import random
import struct
import zlib

import oracle_binding as ob

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "ref_inputs")
WBITS = {0: -15, 1: 15, 2: 31}


def zlib_accepts(stream, data, wrapper):
    """Does zlib inflate `stream` to exactly `data`, reach the end of the stream and leave nothing over?"""
    d = zlib.decompressobj(WBITS[wrapper])
    try:
        out = d.decompress(bytes(stream)) + d.flush()
    except zlib.error:
        return False
    return out == bytes(data) and d.eof and d.unused_data == b""


def pg11():
    with open(os.path.join(FIX, "pg11.txt"), "rb") as f:
        return f.read()


def noise(n, seed):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little")


def literal_runs(seed=5):
    """text with literal runs of 63, 64, 65, 128 and 129 bytes between matches: noise (no match inside a run) between copies of
    one phrase (a match each)"""
    rnd = random.Random(seed)
    phrase = b"the quick brown fox jumps over the lazy dog; "
    out = bytearray(phrase)
    for run in (63, 64, 65, 128, 129, 1, 2, 63, 64, 65):
        out += bytes(rnd.sample(range(128, 256), 100) + rnd.sample(range(128, 256), 100))[:run] + phrase
    return bytes(out)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes; `main` inputs get every stream variant, the others a few"""
    text = pg11()
    r = noise(32768, 11)
    d = {
        "pg11": text,
        "pg11_20000": text[:20000],
        "empty": b"",
        "one_byte": b"Q",
        "noise_200k": noise(200000, 3),
        "zeros_70000": bytes(70000),
        "dist_32768": r + r[:300],
        "literal_runs": literal_runs(),
    }
    main = list(d)
    for p in sorted(glob.glob(os.path.join(FIX, "*")) + glob.glob(os.path.join(FIX, "afl", "*"))):
        if os.path.isfile(p) and not p.endswith("pg11.txt"):
            with open(p, "rb") as f:
                d["fix:" + os.path.relpath(p, FIX)] = f.read()
    import header_cases  # (read only: the inputs that force 15-bit codes and the length limiters)
    for name, data, _level, _target in header_cases.cases():
        d["hdr:" + name] = bytes(data)
    return d, main


GZ_HEADERS = {
    "blank": bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff]),
    "name": bytes([0x1f, 0x8b, 8, 8, 1, 2, 3, 4, 0, 3]) + b"file.txt\0",
    "all": None,  # FEXTRA + FNAME + FCOMMENT + FHCRC, made below
}


def _gz_all():
    h = bytes([0x1f, 0x8b, 8, 2 | 4 | 8 | 16, 9, 8, 7, 6, 2, 3]) + struct.pack("<H", 6) + b"AB\x02\x00xy" + b"n\0" + b"a comment\0"
    return h + struct.pack("<H", zlib.crc32(h) & 0xFFFF)


GZ_HEADERS["all"] = _gz_all()


def gzip_frame(raw, data, header):
    return header + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def _z(data, level, wbits, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def streams():
    """(a): [(name, stream, input, wrapper, table or None)] -- all valid"""
    d, main = inputs()
    out = []
    zl = [("z0", 0, zlib.Z_DEFAULT_STRATEGY), ("z1", 1, zlib.Z_DEFAULT_STRATEGY), ("z6", 6, zlib.Z_DEFAULT_STRATEGY),
          ("z9", 9, zlib.Z_DEFAULT_STRATEGY), ("zfixed", 6, zlib.Z_FIXED), ("zhuff", 6, zlib.Z_HUFFMAN_ONLY), ("zrle", 6, zlib.Z_RLE)]
    for name, data in d.items():
        is_main = name in main
        for zn, level, strat in (zl if is_main else zl[2:3]):
            raw = _z(data, level, -15, strat)
            out.append(("%s/%s/raw" % (name, zn), raw, data, 0, None))
            if is_main:
                out.append(("%s/%s/zlib" % (name, zn), _z(data, level, 15, strat), data, 1, None))
                out.append(("%s/%s/gzip" % (name, zn), _z(data, level, 31, strat), data, 2, None))
        levels = (ob.FAST, ob.DEFAULT, ob.BEST, ob.RLE, ob.HUFFMAN_ONLY) if is_main else (ob.DEFAULT,)
        for lv in levels:
            try:
                raw = ob.encode(data, level=lv)
            except ob.RefPanic:
                continue
            table = [(b["bit_start"], b["in_bytes"]) for b in ob.trace_blocks()]
            trace = [b["btype"] for b in ob.trace_blocks()]
            if not zlib_accepts(raw, data, 0):
                continue  # (the reference's own invalid streams, SURVEY A.4 Q13: a case of the GPU test, not of this list)
            out.append(("%s/o%d/raw" % (name, lv), raw, data, 0, (table, trace)))
            if is_main:
                out.append(("%s/o%d/zlib" % (name, lv), ob.encode(data, level=lv, wrapper=1), data, 1, None))
                for hn, h in GZ_HEADERS.items():
                    if hn == "blank" or lv == ob.DEFAULT:
                        out.append(("%s/o%d/gzip_%s" % (name, lv, hn), gzip_frame(raw, data, h), data, 2, None))
    return out


def mutation_base():
    """the raw and the zlib stream (b) mutates: the 20 000-byte prefix with a full flush in the middle, so that the stream holds a
    stored header with pad bits in front of its LEN as well as the pad behind the BFINAL block"""
    data = pg11()[:20000]
    res = []
    for wrapper in (0, 1):
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrapper])
        first = c.compress(data[:9000]) + c.flush(zlib.Z_FULL_FLUSH)
        res.append((first + c.compress(data[9000:]) + c.flush(), data, wrapper, len(first)))
    return res


@functools.lru_cache(maxsize=None)
def mutations(seed=20240607):
    """(b): [(name, stream, input, wrapper)]"""
    out = []
    for base, data, wrapper, marker_end in mutation_base():
        tag = "raw" if wrapper == 0 else "zlib"
        rnd = random.Random(seed + wrapper)
        flips = set(rnd.sample(range(8 * len(base)), 600))
        # every pad bit: all bits of the byte in front of the stored LEN (marker_end - 5: header bits and pad share it) and of the
        # last deflate byte (in front of the zlib trailer)
        last = len(base) - 1 - (4 if wrapper else 0)
        pad = [8 * (marker_end - 5) + k for k in range(8)] + [8 * last + k for k in range(8)]
        for b in sorted(flips) + pad:
            m = bytearray(base)
            m[b >> 3] ^= 1 << (b & 7)
            out.append(("%s/flip%d%s" % (tag, b, "p" if b in pad else ""), bytes(m), data, wrapper))
        for k in range(1, 10):
            out.append(("%s/trunc%d" % (tag, k), base[:-k], data, wrapper))
        out.append(("%s/append1" % tag, base + b"\0", data, wrapper))
        out.append(("%s/append4" % tag, base + b"\0\1\2\3", data, wrapper))
        if wrapper:
            for k in range(1, 5):
                m = bytearray(base)
                m[-k] ^= 0x5A
                out.append(("%s/trailer%d" % (tag, k), bytes(m), data, wrapper))
    return out


# ---- (c): a bit writer and the streams made with it -------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):  # a field: least significant bit first
        self.bits += [(value >> k) & 1 for k in range(n)]
        return self

    def code(self, value, n):  # a Huffman code: most significant bit first
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def raw(self, data):
        for byte in data:
            self.put(byte, 8)
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lens):
    """code of every symbol with a length (RFC 1951 3.2.2), without checking that the set is complete"""
    code, codes = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def fixed_ll(w, sym):
    if sym < 144:
        return w.code(0x30 + sym, 8)
    if sym < 256:
        return w.code(0x190 + sym - 144, 9)
    if sym < 280:
        return w.code(sym - 256, 7)
    return w.code(0xC0 + sym - 280, 8)


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code: 13/16 + 6/32


def dynamic_header(w, ops, hlit, hdist, bfinal=1):
    """ops: code-length symbols, 16/17/18 as (symbol, extra value)"""
    w.put(bfinal, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for op in ops:
        s, extra = op if isinstance(op, tuple) else (op, None)
        w.code(*cl[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    return w


def _ll(lens_by_symbol, n):
    return [lens_by_symbol.get(s, 0) for s in range(n)]


def dyn_block(ll, dist, body, hdist=None):
    """a final dynamic block: ll / dist = {symbol: length}; body = ll symbols, a distance symbol as ('d', symbol)"""
    ll_l, d_l = _ll(ll, 258), _ll(dist, hdist or max(list(dist) + [0]) + 1)
    w = dynamic_header(BitWriter(), ll_l + d_l, 258, len(d_l))
    lc, dc = canonical(ll_l), canonical(d_l)
    for s in body:
        if isinstance(s, tuple):
            w.code(*dc[s[1]])
        else:
            w.code(*lc[s])
    return w.bytes()


@functools.lru_cache(maxsize=None)
def hand():
    """(c): [(name, stream, input, wrapper, status name)]"""
    A = ord("a")
    r = noise(32768, 17)
    out = []

    def add(name, stream, data, status):
        out.append((name, bytes(stream), bytes(data), 0, status))

    add("btype3", BitWriter().put(1, 1).put(3, 2).bytes(), b"", "BTYPE")
    add("stored_len_nlen", BitWriter().put(1, 1).put(0, 2).align().put(3, 16).put(~3 & 0xFFFF ^ 1, 16).raw(b"abc").bytes(), b"abc", "STORED")
    w = fixed_ll(BitWriter().put(1, 1).put(1, 2), A)
    fixed_ll(w, 257).code(1, 5)  # length 3, distance 2 with one byte produced
    add("distance_one_past_the_start", fixed_ll(w, 256).bytes(), b"aaaa", "DISTANCE")
    # The largest distance the format can write is 32768 (code 29 with its 13 extra bits set): 32769 has no encoding.  The two
    # cases around that edge: distance 32768 at output position 32768 (legal) and at 32767 (one more than was produced).
    for name, n, status in (("distance_32768_at_32768", 32768, "OK"), ("distance_32768_at_32767", 32767, "DISTANCE")):
        w = BitWriter().put(0, 1).put(0, 2).align().put(n, 16).put(~n & 0xFFFF, 16).raw(r[:n]).put(1, 1).put(1, 2)
        fixed_ll(w, 257).code(29, 5).put(8191, 13)
        add(name, fixed_ll(w, 256).bytes(), r[:n] + r[:3], status)
    add("ll_symbol_286", fixed_ll(fixed_ll(BitWriter().put(1, 1).put(1, 2), A), 286).bytes(), b"a", "CODE")
    w = BitWriter().put(1, 1).put(1, 2)
    for _ in range(3):
        fixed_ll(w, A)
    add("distance_symbol_30", fixed_ll(fixed_ll(w, 257).code(30, 5), 256).bytes(), b"aaaaaa", "CODE")
    add("repeat_16_first", dynamic_header(BitWriter(), [(16, 0)] + [8] * 255, 257, 1).bytes(), b"", "LENGTHS")
    add("repeat_overrun", dynamic_header(BitWriter(), [8] * 250 + [(18, 127)], 257, 1).bytes(), b"", "LENGTHS")
    add("ll_over_subscribed", dyn_block({A: 1, A + 1: 1, 256: 1}, {0: 1}, [A, 256]), b"a", "LENGTHS")
    add("ll_incomplete", dyn_block({A: 2, 256: 2}, {0: 1}, [A, 256]), b"a", "LENGTHS")
    add("dist_over_subscribed", dyn_block({A: 1, 256: 2, 257: 2}, {0: 1, 1: 1, 2: 1}, [A, 256]), b"a", "LENGTHS")
    add("dist_incomplete", dyn_block({A: 1, 256: 2, 257: 2}, {0: 2, 1: 2}, [A, 256]), b"a", "LENGTHS")
    add("one_code_dist_set", dyn_block({A: 1, 256: 2, 257: 2}, {0: 1}, [A, A, A, 257, ("d", 0), 256]), b"aaaaaa", "OK")
    add("one_code_ll_set", dyn_block({256: 1}, {}, [256], hdist=1), b"", "OK")
    add("no_distance_codes_no_match", dyn_block({A: 1, 256: 2, 257: 2}, {}, [A, 256], hdist=1), b"a", "OK")
    add("no_distance_codes_match", dyn_block({A: 1, 256: 2, 257: 2}, {}, [A, A, A, 257], hdist=1), b"aaaaaa", "CODE")
    add("no_symbol_256", dyn_block({A: 1, A + 1: 1}, {0: 1}, [A]), b"a", "LENGTHS")
    add("hlit_287", BitWriter().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(15, 4).raw(bytes(40)).bytes(), b"", "LENGTHS")
    w = fixed_ll(fixed_ll(BitWriter().put(0, 1).put(1, 2), A), 256)
    add("bfinal_missing", w.bytes(), b"a", "TRUNCATED")
    add("token_past_in_len", fixed_ll(fixed_ll(fixed_ll(BitWriter().put(1, 1).put(1, 2), A), A), 256).bytes(), b"a", "LENGTH")
    add("bfinal_before_in_len", fixed_ll(fixed_ll(BitWriter().put(1, 1).put(1, 2), A), 256).bytes(), b"ab", "LENGTH")
    # literal runs of exactly 63, 64, 65, 128 and 129 between matches (the decoder compares its literals 64 at a time)
    w, data, rnd = BitWriter().put(1, 1).put(1, 2), bytearray(), random.Random(23)
    for run in (63, 64, 65, 128, 129, 1, 64):
        lits = bytes(rnd.getrandbits(8) for _ in range(run))
        for c in lits:
            fixed_ll(w, c)
        fixed_ll(w, 257).code(0, 5)  # length 3, distance 1
        data += lits + lits[-1:] * 3
    add("literal_runs_exact", fixed_ll(w, 256).bytes(), data, "OK")
    add("literal_differs", fixed_ll(fixed_ll(BitWriter().put(1, 1).put(1, 2), A), 256).bytes(), b"b", "MISMATCH")
    return out


@functools.lru_cache(maxsize=None)
def edits():
    """(d): [(name, stream, edited input, wrapper, k)] -- byte k of the input changed under a valid stream"""
    data = pg11()[:20000]
    stream = ob.encode(data, level=ob.DEFAULT)
    pos, lit, inside, source = 0, None, None, None
    for t in ob.lz77(data, 128, 32, 1):
        n = 1 if t[0] == "lit" else t[1]
        if t[0] == "lit" and pos > 0 and lit is None:
            lit = pos
        if t[0] == "ld" and source is None:
            source = pos - t[2]
        if t[0] == "ld" and n >= 20 and inside is None:
            inside = pos + n // 2
        pos += n
    out = []
    for name, k in (("first", 0), ("literal", lit), ("inside_match", inside), ("match_source", source), ("last", len(data) - 1)):
        m = bytearray(data)
        m[k] ^= 0x20
        out.append((name, stream, bytes(m), 0, k))
    return out


def corpus():
    """every (stream, input, wrapper, table) of the four groups: what the sanitizer program runs over"""
    for _name, s, d, w, tab in streams():
        yield s, d, w, None
        if tab:
            yield s, d, w, tab[0]
    for c in mutations():
        yield c[1], c[2], c[3], None
    for c in hand():
        yield c[1], c[2], c[3], None
    for c in edits():
        yield c[1], c[2], c[3], None
