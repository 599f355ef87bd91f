"""Cases for the inflate index (include/mi355_deflate.h mi355_inflate_index*, mi355_inflate_parallel*): seeded, shared by the CPU
test of the host build (test_inflate_index_cases.py) and the GPU test (test_inflate_index_gpu.py).  TEST INFRASTRUCTURE.

  (a) streams()    what a decoder meets: text at zlib's levels, the oracle's streams, cut streams with an empty stored block between
                   dynamic blocks, streams assembled bit by bit for the places zlib does not reach (every bit phase of a block start,
                   a candidate at the first and at the last bit of a span, a header across a span edge and across the stream's end),
                   fixed only, stored only, Huffman only, RLE, a megabyte of zeros, nothing, one byte, zlib and gzip frames
  (b) decoys()     a stored block whose payload holds a valid non-final dynamic block: in front of a true boundary of the same span,
                   and ending exactly where the stored block ends
  (c) mutated()    bit flips and truncations inside the first, a middle and the last link at S = 256; a first match with dist > p
  (d) caps         short buffers around every entry seam, and the size query

A case is a Case tuple.  `want` is what zlib inflates the stream to, None if zlib refuses it: the judge is zlib alone.  `starts` are
bit offsets (raw deflate) at which a non-final dynamic block is KNOWN to begin -- from trace_blocks(), from a cut stream's table or
from the writer that assembled the stream --, `complete` says that no other exists.  Every precondition a case is named for is
asserted on the host build by test_inflate_index_cases.py with the facts kept in `facts`.
"""
import collections
import functools
import random
import zlib

import datagen
import inflate_table_cases as tc
import verify_cases as vc

Case = collections.namedtuple("Case", "name stream wrapper want starts complete facts")

SPANS = (256, 4096, None)  # None: the default of MI355_CFG_INFLATE_INDEX_SPAN_BYTES
A, B = ord("a"), ord("b")
ZCUT_SEED = 1  # (the test asserts that this seed's cuts put a stored block's front on every bit phase)


def head_bits(raw, bit):
    """BFINAL | BTYPE << 1 at a bit offset of a raw stream"""
    return sum(((raw[(bit + k) >> 3] >> ((bit + k) & 7)) & 1) << k for k in range(3))


def dynamic_starts(raw, bits):
    """those of the block starts `bits` at which a non-final dynamic block begins"""
    return [b for b in bits if head_bits(raw, b) == 4]


# ---- a writer of dynamic blocks: 'a' is one bit, 'b' and the end of the block two -----------------------------------------------
def cl_ops(lens):
    """the code-length symbols that spell `lens`: zero runs as 18 / 17, everything else as itself"""
    ops, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            n = 0
            while i + n < len(lens) and lens[i + n] == 0:
                n += 1
            i += n
            while n >= 11:
                k = min(n, 138)
                ops.append((18, k - 11))
                n -= k
            if n >= 3:
                ops.append((17, n - 3))
                n = 0
            ops += [0] * n
        else:
            ops.append(lens[i])
            i += 1
    return ops


LL = {A: 1, B: 2, 256: 2}
LL_LENS = [LL.get(s, 0) for s in range(257)]
LL_CODES = vc.canonical(LL_LENS)
DYN_OPS = cl_ops(LL_LENS + [1])


def dyn(w, text, bfinal=0):
    """a dynamic block of the letters a / b; returns the bit at which it begins"""
    at = len(w.bits)
    vc.dynamic_header(w, DYN_OPS, 257, 1, bfinal)
    for ch in text:
        w.code(*LL_CODES[ch])
    w.code(*LL_CODES[256])
    return at


DYN_BITS = (lambda w: (dyn(w, b""), len(w.bits))[1])(vc.BitWriter())  # bits of a block without letters: header + end of block


def dyn_until(w, end_bit, bfinal=0):
    """a dynamic block of a's that ends exactly at end_bit"""
    n = end_bit - len(w.bits) - DYN_BITS
    assert n >= 0, "no room for a block"
    at = dyn(w, b"a" * n, bfinal)
    assert len(w.bits) == end_bit
    return at, n


def stored(w, data, bfinal=0):
    at = len(w.bits)
    w.put(bfinal, 1).put(0, 2).align().put(len(data), 16).put(~len(data) & 0xFFFF, 16).raw(data)
    return at


def hand_phases():
    """non-final dynamic blocks that begin at every bit phase, each in a span of 256 bytes of its own; the last block is final"""
    w, data, starts = vc.BitWriter(), b"", []
    for k, phase in enumerate((0, 1, 2, 3, 4, 5, 6, 7, 0)):
        end = 2048 * 2 * (k + 1) + phase  # (two spans a block: a start in every other span)
        at, n = dyn_until(w, end)
        starts.append(at)
        data += b"a" * n
    dyn(w, b"ab", 1)
    data += b"ab"
    assert {s % 8 for s in starts} == set(range(8))
    return w.bytes(), data, starts


def hand_span_edges():
    """a stored block, then dynamic blocks that begin at the FIRST bit of span 1 (S = 256), at the LAST bit of span 3, and 40 bits in
    front of span 6 (the header lies across the edge); a's are zero bits, so no span holds anything else"""
    w = vc.BitWriter()
    fill = vc.noise(251, 61)
    stored(w, fill)  # 1 + 4 + 251 bytes
    data = fill
    s1, n = dyn_until(w, 2048 * 4 - 1)
    data += b"a" * n
    s2, n = dyn_until(w, 2048 * 6 - 40)
    data += b"a" * n
    s3, n = dyn_until(w, 2048 * 8 + 13)
    data += b"a" * n
    dyn(w, b"ba", 1)
    data += b"ba"
    assert (s1, s2, s3) == (2048, 2048 * 4 - 1, 2048 * 6 - 40)
    return w.bytes(), data, [s1, s2, s3]


def hand_decoy(exact):
    """(b) of the module's text.  exact False: A | stored[ decoy block, BTYPE 3 ] | D | E | F with the decoy and D in span 1 (S = 256);
    exact True: A | stored[ decoy block that ends where the payload ends, in span 2 ] | D | F"""
    w = vc.BitWriter()
    data = b""
    _a, n = dyn_until(w, 2048 + 301)
    data += b"a" * n
    p = vc.BitWriter()
    if exact:
        dyn_until(p, 8 * 300)  # (the block's end is the payload's: byte aligned, beyond the edge at 2048 * 2)
    else:
        dyn(p, b"ab" * 10)
        p.put(0, 1).put(3, 2)
    payload = p.bytes()
    s_at = stored(w, payload)
    decoy = len(w.bits) - 8 * len(payload)
    data += payload
    facts = dict(decoy=decoy, stored=s_at)
    d_at, n = dyn_until(w, 2048 * 3 + 77 if not exact else 2048 * 4 + 5)
    data += b"a" * n
    starts = [0, d_at]
    if not exact:
        e_at, n = dyn_until(w, 2048 * 5 + 3)
        data += b"a" * n
        starts.append(e_at)
        facts["e"] = e_at
    dyn(w, b"bb", 1)
    data += b"bb"
    facts["d"] = d_at
    return w.bytes(), data, starts, facts


def hand_distance(first):
    """a fixed block whose first match reaches in front of the stream (the index cannot see it), then dynamic blocks in later spans"""
    w = vc.BitWriter()
    w.put(0, 1).put(1, 2)
    if not first:
        for ch in b"xy":
            vc.fixed_ll(w, ch)
    tc.fixed_match(w, 5, 3)
    vc.fixed_ll(w, 256)
    for k in (2, 4, 6):
        dyn_until(w, 2048 * k + 9)
    dyn(w, b"ab", 1)
    return w.bytes()


def _z(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


# ---- (a), (b) ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streams():
    out = []

    def add(name, stream, wrapper=0, starts=None, complete=False, facts=None, want=False):
        want = tc.zlib_out(stream, wrapper) if want is False else want
        out.append(Case(name, bytes(stream), wrapper, want, starts, complete, facts or {}))

    text = datagen.text_like(1 << 20, 20261018)
    for level in (1, 6, 9):
        add("text/l%d" % level, _z(text, level))
    for c in tc.oracle():
        if c.gbytes != tc.GROUP_DEFAULT or c.wrapper:
            continue
        add(c.name.replace("oracle:", "oracle/"), c.stream, 0, dynamic_starts(c.stream, [b for b, _n in c.table]), True)
    # cut streams: every entry shorter than zlib's symbol buffer, so an entry is ONE block and the flush's empty stored block; the
    # boundaries in front of the stored blocks fall on every bit phase
    data = vc.pg11()[:150000]
    rnd = random.Random(ZCUT_SEED)
    lens = []
    while sum(lens) < len(data):
        lens.append(min(rnd.randrange(3000, 9000), len(data) - sum(lens)))
    raw, table = tc.zcut(data, lens)
    add("zcut/phases", raw, 0, dynamic_starts(raw, [b for b, _n in table]), True, dict(entries=[b for b, _n in table]))
    raw, data, starts = hand_phases()
    add("hand/phases", raw, 0, starts, True)
    cut = (starts[3] + 60) // 8  # inside the header of a block that begins in a span of its own
    add("hand/header_across_the_end", raw[:cut], 0, starts[:3], True, dict(header=starts[3]))
    raw, data, starts = hand_span_edges()
    add("hand/span_edges", raw, 0, starts, True)
    text = vc.pg11()
    add("fixed", _z(text * 2, 6, zlib.Z_FIXED), 0, [], True)
    add("stored", _z(vc.noise(200000, 67), 0), 0, [], True)
    add("huffman_only", _z(text * 2, 6, zlib.Z_HUFFMAN_ONLY))
    add("rle", _z(text * 2, 6, zlib.Z_RLE))
    add("zeros_1m", _z(bytes(1 << 20), 9))
    add("empty", b"")
    add("one_byte", b"\x03")
    add("zlib", _z(text * 3, 6, wbits=15), 1)
    add("gzip_name_extra", vc.gzip_frame(_z(text * 3, 1), text * 3, vc.GZ_HEADERS["all"]), 2)
    for name, exact in (("decoy/a", False), ("decoy/b", True)):
        raw, data, starts, facts = hand_decoy(exact)
        add(name, raw, 0, starts, True, facts)
    return out


def by_name(name):
    return [c for c in streams() if c.name == name][0]


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
MUTATION_BASE = "oracle/pg11x3/fast/w0"


def mutated(links, seed=20261018):
    """links: [(first bit, end bit)] of the base stream's entries at S = 256 (the host build's table).  Seeded bit flips and
    truncations inside the first, a middle and the last one, and the two streams whose first match reaches in front of the stream."""
    raw = by_name(MUTATION_BASE).stream
    rnd = random.Random(seed)
    out = []
    for k in sorted({0, len(links) // 2, len(links) - 1}):
        lo, hi = links[k]
        for b in sorted(rnd.sample(range(lo, hi), 24)) + [lo, lo + 1, lo + 2, hi - 1]:
            m = bytearray(raw)
            m[b >> 3] ^= 1 << (b & 7)
            out.append(Case("mutated/flip%d@%d" % (b, k), bytes(m), 0, tc.zlib_out(bytes(m), 0), None, False, {}))
        for cut_at in sorted(rnd.sample(range(lo // 8 + 1, hi // 8), 3)):
            out.append(Case("mutated/trunc%d@%d" % (cut_at, k), raw[:cut_at], 0, tc.zlib_out(raw[:cut_at], 0), None, False, {}))
    for first in (True, False):
        s = hand_distance(first)
        out.append(Case("mutated/distance_%s" % ("first_token" if first else "third_token"), s, 0, tc.zlib_out(s, 0), None, False, {}))
    return out
