"""Cases for the tabled inflate (include/mi355_deflate.h mi355_inflate_tabled*): seeded, shared by the CPU test of the host builds
(test_inflate_table_cases.py) and the GPU test (test_inflate_table_gpu.py).  TEST INFRASTRUCTURE.

  (a) oracle()     the oracle's streams with their trace_blocks() tables: three copies of pg11.txt at every level, noise, one entry
  (b) cut()        Python zlib streams cut with Z_SYNC_FLUSH at chosen input offsets -- entry k is (8 * len(output so far), bytes
                   since the last cut), from zlib alone -- and two streams assembled bit by bit for what zlib never writes
  (c) wrong()      valid streams with tables that are wrong
  (d) mutated()    bit flips and truncations inside the first, a middle and the last entry
  (e) caps()       short buffers: every case of corpus() names the buffer sizes it is to be run with

A case is a Case tuple; `want` is what zlib inflates the stream to, None if zlib refuses it.  The judge is zlib alone.
"""
import collections
import functools
import random
import struct
import zlib

import oracle_binding as ob
import verify_cases as vc

Case = collections.namedtuple("Case", "name group stream wrapper table want gbytes caps")

GROUP_DEFAULT = 256 << 20
GROUP_MIN = 64 << 10


def zlib_out(stream, wrapper):
    """what zlib inflates the stream to, if it takes all of it and nothing is left over; else None"""
    d = zlib.decompressobj(vc.WBITS[wrapper])
    try:
        out = d.decompress(bytes(stream)) + d.flush()
    except zlib.error:
        return None
    return out if d.eof and d.unused_data == b"" else None


def total(table):
    return sum(n for _bit, n in table)


def starts(table):
    """the output position at which every entry begins"""
    out, p = [], 0
    for _bit, n in table:
        out.append(p)
        p += n
    return out


def default_cap(c):
    """the buffer a case is run with first: zlib's length; for a stream zlib refuses, what the table promises"""
    if c.want is not None:
        return len(c.want)
    return total(c.table) or 20000


def frame(raw, data, wrapper):
    if wrapper == 0:
        return raw
    if wrapper == 1:
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)
    return vc.gzip_frame(raw, data, vc.GZ_HEADERS["name"])


def seam_caps(table, n):
    """(e): 0, 1, one less than the size, the size, inside entry 0, on an entry seam, one beyond a seam"""
    st = [p for p in starts(table) if 0 < p < n]
    caps = {0, 1, n - 1, n}
    if st:
        caps |= {st[0] // 2, st[0], st[0] + 1, st[-1], st[-1] + 1}
    return sorted(c for c in caps if 0 <= c <= n)


def pg11x3():
    return vc.pg11() * 3


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    out = []
    text = pg11x3()
    levels = (("fast", ob.FAST), ("default", ob.DEFAULT), ("best", ob.BEST), ("rle", ob.RLE), ("huffman_only", ob.HUFFMAN_ONLY))
    for inp, data, lvs in (("pg11x3", text, levels), ("noise_200k", vc.noise(200000, 3), levels[1:2]),
                           ("one_entry", vc.pg11()[:20000], levels[1:2])):
        for lname, lv in lvs:
            raw = ob.encode(data, level=lv)
            table = [(b["bit_start"], b["in_bytes"]) for b in ob.trace_blocks()]
            assert zlib_out(raw, 0) == data
            for wrapper in ((0, 1, 2) if lname == "default" else (0,)):
                for gname, g in (("", GROUP_DEFAULT), ("/g64k", GROUP_MIN)):
                    if g == GROUP_MIN and (inp != "pg11x3" or (wrapper and lname != "default")):
                        continue
                    caps = seam_caps(table, len(data)) if (lname, wrapper) == ("default", 0) else []
                    out.append(Case("oracle:%s/%s/w%d%s" % (inp, lname, wrapper, gname), "oracle", frame(raw, data, wrapper), wrapper,
                                    table, data, g, caps))
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def zcut(data, lens, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """(raw stream, table) of `data` compressed by zlib and cut behind every lens[k] input bytes.  A cut is Z_SYNC_FLUSH; an entry
    of no bytes behind another cut is Z_FULL_FLUSH, the flush that writes an (empty stored) block although nothing came in."""
    assert sum(lens) == len(data)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, table, pos = b"", [], 0
    for k, n in enumerate(lens):
        start = 8 * len(out)
        out += c.compress(data[pos:pos + n])
        pos += n
        if k == len(lens) - 1:
            out += c.flush()
        else:
            out += c.flush(zlib.Z_FULL_FLUSH if n == 0 and k > 0 else zlib.Z_SYNC_FLUSH)
        assert 8 * len(out) > start, "an entry owns a block at least"
        table.append((start, n))
    return out, table


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def fixed_match(w, length, dist):
    """a match in the fixed code"""
    i = 28 if length == 258 else max(k for k in range(28) if LBASE[k] <= length)
    vc.fixed_ll(w, 257 + i).put(length - LBASE[i], LEXT[i])
    j = max(k for k in range(30) if DBASE[k] <= dist)
    return w.code(j, 5).put(dist - DBASE[j], DEXT[j])


def hand_first_byte():
    """What zlib never writes (its longest distance is 32768 - 262): the FIRST token of an entry is a match of distance 32768, and of
    the next entry a match of distance 1 -- both sources are the window in front of the entry, its first and its last byte."""
    r = vc.noise(32768, 29)
    w = vc.BitWriter()
    table, data = [], bytearray()

    def entry(n_before):
        table.append([len(w.bits), 0])
        return n_before

    at = entry(0)
    w.put(0, 1).put(0, 2).align().put(32768, 16).put(~32768 & 0xFFFF, 16).raw(r)
    data += r
    table[-1][1] = len(data) - at
    at = entry(len(data))
    fixed_match(w.put(0, 1).put(1, 2), 20, 32768)
    data += data[-32768:-32768 + 20]
    for ch in b"xyz":
        vc.fixed_ll(w, ch)
    data += b"xyz"
    vc.fixed_ll(w, 256)
    table[-1][1] = len(data) - at
    at = entry(len(data))
    fixed_match(w.put(1, 1).put(1, 2), 258, 1)
    data += b"z" * 258
    fixed_match(w, 70, 32768)
    for _ in range(70):
        data.append(data[-32768])
    vc.fixed_ll(w, 256)
    table[-1][1] = len(data) - at
    return w.bytes(), [tuple(t) for t in table], bytes(data)


@functools.lru_cache(maxsize=None)
def cut():
    out = []
    text = vc.pg11()

    def add(name, raw, table, data, caps=False, groups=(GROUP_DEFAULT,), wrappers=(0,)):
        assert zlib_out(raw, 0) == data, name
        for wrapper in wrappers:
            for g in groups:
                out.append(Case("cut:%s/w%d%s" % (name, wrapper, "/g64k" if g == GROUP_MIN else ""), "cut", frame(raw, data, wrapper),
                                wrapper, table, data, g, seam_caps(table, len(data)) if caps and not wrapper and g == GROUP_DEFAULT else []))

    # entry lengths 0, 1, 63, 64, 65, 32767, 32768, 32769, 40000 (and 0 in front of everything): text, so that matches cross the cuts
    lens = [0, 40000, 1, 63, 0, 64, 65, 32767, 32768, 32769, 5000]
    data = (text * 2)[3000:3000 + sum(lens)]
    raw, table = zcut(data, lens)
    add("lengths", raw, table, data, caps=True, groups=(GROUP_DEFAULT, GROUP_MIN), wrappers=(0, 1, 2))
    # one random block of 20 000 bytes, eight times, an entry each: every entry is copies of the one in front of it
    block = vc.noise(20000, 41)
    raw, table = zcut(block * 8, [20000] * 8, level=9)
    add("copies_of_copies", raw, table, block * 8, groups=(GROUP_DEFAULT, GROUP_MIN))
    # a distance-1 run across a cut
    data = text[:5000] + b"z" * 3000 + text[5000:9000]
    raw, table = zcut(data, [6500, len(data) - 6500])
    add("run_across_a_cut", raw, table, data)
    # stored pieces at every destination alignment mod 8 (level 0: every entry is stored pieces), one of them longer than a piece
    lens = [1001] * 9 + [70001, 7, 8, 9, 3]
    data = vc.noise(sum(lens), 43)
    raw, table = zcut(data, lens, level=0)
    assert {p % 8 for p in starts(table)} == set(range(8))
    add("stored_alignments", raw, table, data, caps=True)
    raw, table, data = hand_first_byte()
    add("first_byte_32768_and_1", raw, table, data, caps=True)
    return out


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mutation_base():
    """60 000 bytes of text in three entries of 20 000"""
    data = vc.pg11()[1000:61000]
    raw, table = zcut(data, [20000, 20000, 20000])
    return raw, table, data


def refused(table):
    """is the table MI355_E_ARG from its numbers alone?  (bits that do not ascend, a first entry that does not begin at bit 0)"""
    return table[0][0] != 0 or any(table[k][0] > table[k + 1][0] for k in range(len(table) - 1))


WRONG_KINDS = ["bit+1", "bit-1", "bytes+1", "bytes-1", "total+1", "total-1", "dropped", "merged", "bfinal_not_last", "bfinal_not_last_split"]


@functools.lru_cache(maxsize=None)
def wrong():
    """Tables that are wrong, for valid streams of three entries and more: text (matches reach in front of every entry), stored
    entries and Huffman-only entries (nothing reaches in front of an entry: only the table's own rules can notice)."""
    out = []
    bases = [("z3",) + mutation_base()]
    o = [c for c in oracle() if c.name == "oracle:pg11x3/default/w0"][0]
    bases.append(("o", o.stream, o.table, o.want))
    data = vc.noise(60000, 47)
    bases.append(("s3",) + zcut(data, [20000] * 3, level=0) + (data,))
    data = vc.pg11()[2000:62000]
    bases.append(("h3",) + zcut(data, [20000] * 3, strategy=zlib.Z_HUFFMAN_ONLY) + (data,))
    for bname, raw, table, data in bases:
        n = len(table)
        assert n >= 3
        m = n // 2

        def add(name, t):
            assert all(x[1] >= 0 for x in t), name
            out.append(Case("wrong:%s/%s" % (bname, name), "wrong", raw, 0, [tuple(x) for x in t], data, GROUP_DEFAULT, []))

        for k in sorted({1, m, n - 1}):
            for d in (1, -1):
                t = [list(x) for x in table]
                t[k][0] += d
                add("bit%+d@%d" % (d, k), t)
                t = [list(x) for x in table]
                t[k - 1][1] += d
                t[k][1] -= d
                add("bytes%+d@%d" % (d, k), t)
        for d in (1, -1):
            t = [list(x) for x in table]
            t[-1][1] += d
            add("total%+d" % d, t)
        for k in sorted({0, m, n - 1}):
            add("dropped@%d" % k, [list(x) for j, x in enumerate(table) if j != k])  # (@0: the first entry no longer begins at bit 0)
            if k:  # ... with its bytes given to the entry in front of it: a coarser table, and a right one
                t = [list(x) for j, x in enumerate(table) if j != k]
                t[k - 1][1] += table[k][1]
                add("merged@%d" % k, t)
        add("bfinal_not_last", [list(x) for x in table] + [[8 * len(raw), 0]])
        add("bfinal_not_last_split", [list(x) for x in table[:-1]] + [[table[-1][0], table[-1][1] - 5], [8 * len(raw), 5]])
    return out


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mutated(seed=20241018):
    """verify_cases.mutations()' method on a stream of three entries: seeded bit flips and truncations inside entry 0, the middle
    entry and the last one"""
    raw, table, _data = mutation_base()
    rnd = random.Random(seed)
    out = []
    ends = [t[0] for t in table[1:]] + [8 * len(raw)]
    for k, (bit, _n) in enumerate(table):
        for b in sorted(rnd.sample(range(bit, ends[k]), 40)) + [bit, bit + 1, bit + 2, ends[k] - 1]:
            m = bytearray(raw)
            m[b >> 3] ^= 1 << (b & 7)
            out.append(Case("mutated:flip%d@%d" % (b, k), "mutated", bytes(m), 0, table, zlib_out(bytes(m), 0), GROUP_DEFAULT, []))
        for cut_at in sorted(rnd.sample(range(bit // 8 + 1, ends[k] // 8), 3)):
            m = raw[:cut_at]
            out.append(Case("mutated:trunc%d@%d" % (cut_at, k), "mutated", m, 0, table, zlib_out(m, 0), GROUP_DEFAULT, []))
    # a trailer that is wrong, and bytes behind it
    c = [c for c in cut() if c.name == "cut:lengths/w1"][0]
    for name, s in (("adler", c.stream[:-2] + bytes([c.stream[-2] ^ 0x40]) + c.stream[-1:]), ("byte_behind", c.stream + b"\0")):
        out.append(Case("mutated:zlib_%s" % name, "mutated", s, 1, c.table, None, GROUP_DEFAULT, []))
    c = [c for c in cut() if c.name == "cut:lengths/w2"][0]
    for name, s in (("crc", c.stream[:-8] + bytes([c.stream[-8] ^ 1]) + c.stream[-7:]), ("isize", c.stream[:-1] + bytes([c.stream[-1] ^ 1])),
                    ("header", b"\x1f\x8c" + c.stream[2:])):
        out.append(Case("mutated:gzip_%s" % name, "mutated", s, 2, c.table, None, GROUP_DEFAULT, []))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    return oracle() + cut() + wrong() + mutated()


def runs():
    """every (case, out_cap) a test is to make: the default buffer of each case, and the caps of (e)"""
    for c in corpus():
        yield c, default_cap(c)
        for cap in c.caps:
            if cap != default_cap(c):
                yield c, cap
