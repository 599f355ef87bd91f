"""Cases for the cuts of a seek handle (include/mi355_deflate.h MI355_CFG_INFLATE_SEEK_CUT_BYTES, deflate-rs_amd/csrc/inflate_cut.h):
seeded, shared by the CPU test of the host build (test_inflate_cut_cases.py) and the GPU test (test_inflate_cut_gpu.py).
TEST INFRASTRUCTURE.

The judge of bytes is zlib, sliced.  The judge of a cut list is walk(): a plain Python walk of the stream -- a bit reader, the two
Huffman decodes and the cut rule -- that shares no text with the C++.  It also says what every cut lands on and where every match
of a cut has its source, which is what CELLS is counted from: every case names the cells it is there for and coverage() asserts
that the walk reaches them.

  text      zlib -6 text cut with Z_SYNC_FLUSH / Z_FULL_FLUSH into entries: one of a single cut, empty ones, one whose length is a
            multiple of every cut_bytes; raw, zlib and gzip
  stored    zlib -0: stored blocks only, ONE entry
  fixed     Z_FIXED: fixed blocks only, ONE entry (its cuts lie inside the blocks: the header of a block behind a Huffman block is
            never a cut, because the end-of-block token in front of it has the same position and is tested first)
  hand      assembled bit by bit: an entry of stored, fixed, stored and dynamic blocks, then behind a point an entry that is one run of distance-1 matches of 258 bytes
            (every symbol a marker, through all its cuts), an entry of matches of periods 7 and 13 whose sources begin in front of
            it, an entry that puts a cut behind 0 .. 63 gathered literals, and a zlib -9 stream of text
"""
import bisect
import collections
import functools
import zlib

import inflate_table_cases as tc
import verify_cases as vc

Case = collections.namedtuple("Case", "name stream raw wrapper table want cells")

WIN = 32768
SPACING = WIN            # points fall inside the streams
CUT_BYTES = (64, 256, 4096)
LIT_RUN = 64
GROUP_DEFAULT, GROUP_MIN = tc.GROUP_DEFAULT, tc.GROUP_MIN

CELLS = ("hdr_stored", "hdr_fixed", "hdr_dynamic", "tok_literal", "tok_match", "tok_eob", "behind_258", "src_same_cut", "src_earlier_cut",
         "src_front_of_entry", "src_straddles_cut", "src_straddles_entry", "one_cut_entry", "empty_entry", "multiple_entry", "all_markers_3_cuts",
         "period_not_64", "every_lit_offset")


# ---- the Python walk ---------------------------------------------------------------------------------------------------------------
def _bits(raw, pos, n):
    return (int.from_bytes(raw[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)


def _code(lens):
    """canonical Huffman code as {(length, code): symbol}"""
    out, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                out[(n, code)] = s
                code += 1
        code <<= 1
    return out


def _sym(raw, pos, code):
    c = 0
    for n in range(1, 16):
        c = c << 1 | _bits(raw, pos + n - 1, 1)
        if (n, c) in code:
            return code[(n, c)], pos + n
    raise AssertionError("no code at bit %d" % pos)


FIXED = (_code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _code([5] * 30))


def _dynamic(raw, pos):
    hlit, hdist, hclen = _bits(raw, pos, 5) + 257, _bits(raw, pos + 5, 5) + 1, _bits(raw, pos + 10, 4) + 4
    pos += 14
    cl = [0] * 19
    for k in range(hclen):
        cl[vc.CL_ORDER[k]] = _bits(raw, pos, 3)
        pos += 3
    clc, lens = _code(cl), []
    while len(lens) < hlit + hdist:
        s, pos = _sym(raw, pos, clc)
        if s < 16:
            lens.append(s)
            continue
        extra, base, val = {16: (2, 3, None), 17: (3, 3, 0), 18: (7, 11, 0)}[s]
        lens += [lens[-1] if val is None else val] * (base + _bits(raw, pos, extra))
        pos += extra
    return (_code(lens[:hlit]), _code(lens[hlit:])), pos


Place = collections.namedtuple("Place", "bit pos hdr kind entry")  # kind: H0 H1 H2 (a header) L M E (a token start)
Match = collections.namedtuple("Match", "pos len dist")


@functools.lru_cache(maxsize=None)
def walk(raw, table):
    """every place of the stream in order, every match, and the stream's end (bit, pos)"""
    pos_of = tc.starts(list(table))
    places, matches, bit, p, e = [], [], 0, 0, -1
    while True:
        if e + 1 < len(table) and table[e + 1][0] == bit:  # (every entry owns a block at least)
            e += 1
            assert pos_of[e] == p
        hdr, final, btype = bit, _bits(raw, bit, 1), _bits(raw, bit + 1, 2)
        places.append(Place(bit, p, hdr, "H%d" % btype, e))
        bit += 3
        if btype == 0:
            bit = (bit + 7) & ~7
            n = _bits(raw, bit, 16)
            assert n ^ _bits(raw, bit + 16, 16) == 0xFFFF
            bit += 32 + 8 * n
            p += n
        else:
            (ll, dd), bit = (FIXED, bit) if btype == 1 else _dynamic(raw, bit)
            while True:
                at = bit
                s, bit = _sym(raw, bit, ll)
                places.append(Place(at, p, hdr, "L" if s < 256 else "E" if s == 256 else "M", e))
                if s < 256:
                    p += 1
                elif s == 256:
                    break
                else:
                    i = s - 257
                    n = tc.LBASE[i] + _bits(raw, bit, tc.LEXT[i])
                    bit += tc.LEXT[i]
                    d, bit = _sym(raw, bit, dd)
                    dist = tc.DBASE[d] + _bits(raw, bit, tc.DEXT[d])
                    bit += tc.DEXT[d]
                    matches.append(Match(p, n, dist))
                    p += n
        if final:
            return tuple(places), tuple(matches), (bit, p)


def cuts(c, cut_bytes):
    """the cut rule over the walk: [(bit, pos, hdr_bit)] in stream order, and per cut what it lands on (the Place)"""
    places, _m, _end = walk(c.raw, tuple(c.table))
    out, on, e, last = [], [], -1, 0
    for pl in places:
        if pl.entry != e:  # the first cut of an entry is its start
            e, last = pl.entry, pl.pos
            out.append((pl.bit, pl.pos, pl.hdr))
            on.append(pl)
        elif pl.pos - last >= cut_bytes:
            last = pl.pos
            out.append((pl.bit, pl.pos, pl.hdr))
            on.append(pl)
    return out, on


def cells(c, cut_bytes):
    """the cells of CELLS that the case reaches at this cut_bytes"""
    places, matches, _end = walk(c.raw, tuple(c.table))
    cl, on = cuts(c, cut_bytes)
    pos_of = tc.starts(c.table)
    got = set()
    index = {(pl.bit, pl.kind[0] == "H"): i for i, pl in enumerate(places)}
    per_entry = collections.Counter(pl.entry for pl in on)
    lit_offsets = set()
    for k, pl in enumerate(on):
        first = k == 0 or on[k - 1].entry != pl.entry
        if first:
            continue  # (an entry's start is a cut with or without the rule)
        got.add({"H0": "hdr_stored", "H1": "hdr_fixed", "H2": "hdr_dynamic", "L": "tok_literal", "M": "tok_match", "E": "tok_eob"}[pl.kind])
        i = index[(pl.bit, pl.kind[0] == "H")]
        run = 0  # literals its predecessor's wave has gathered when it stops here
        while i - 1 - run >= 0 and places[i - 1 - run].kind == "L" and places[i - 1 - run].pos >= on[k - 1].pos and places[i - 1 - run].hdr == pl.hdr:
            run += 1
        if pl.kind != "H" and run:
            lit_offsets.add(run % LIT_RUN)
        if places[i - 1].kind == "M" and pl.pos - places[i - 1].pos == 258 and places[i - 1].pos - on[k - 1].pos < cut_bytes:
            got.add("behind_258")
    if len(lit_offsets | {0}) == LIT_RUN:
        got.add("every_lit_offset")
    starts = sorted(set(x[1] for x in cl))
    for m in matches:
        ck = starts[bisect.bisect_right(starts, m.pos) - 1]  # the cut that holds the match (a match never spans a cut's start)
        ek = pos_of[bisect.bisect_right(pos_of, m.pos) - 1]  # ... and where its entry begins
        a, b = m.pos - m.dist, m.pos - m.dist + min(m.len, m.dist)  # the source [a, b)
        if a >= ck:
            got.add("src_same_cut")
        elif b <= ck and a >= ek:
            got.add("src_earlier_cut")
        elif b <= ek:
            got.add("src_front_of_entry")
        if a < ck < b and ck > ek:
            got.add("src_straddles_cut")
        if a < ek < b:
            got.add("src_straddles_entry")
        if m.dist % 64 and 64 % m.dist and m.len > m.dist and a < ek:
            got.add("period_not_64")
    for e, (_bit, n) in enumerate(c.table):
        if n == 0:
            got.add("empty_entry")
        elif per_entry[e] == 1:
            got.add("one_cut_entry")
        if n and n % cut_bytes == 0:
            got.add("multiple_entry")
        # an entry behind a point whose every byte comes from in front of it, through three cuts at least
        if e and n and per_entry[e] >= 3:
            ms = [m for m in matches if pos_of[e] <= m.pos < pos_of[e] + n]
            if sum(m.len for m in ms) == n and all(m.dist == 1 for m in ms):
                got.add("all_markers_3_cuts")
    return got


def coverage():
    """{cell: [(case, cut_bytes)]} over the corpus; every case reaches the cells it names at one cut_bytes at least"""
    table = {cell: [] for cell in CELLS}
    for c in corpus():
        mine = set()
        for cb in CUT_BYTES:
            for cell in cells(c, cb):
                table[cell].append((c.name, cb))
                mine.add(cell)
        assert set(c.cells) <= mine, (c.name, sorted(set(c.cells) - mine))
    return table


def print_coverage(table):
    for cell in CELLS:
        print("%-22s %3d  %s" % (cell, len(table[cell]), ", ".join("%s@%d" % x for x in table[cell][:4])))


# ---- the streams -------------------------------------------------------------------------------------------------------------------
def _case(name, raw, table, data, wrapper, cells_):
    assert tc.zlib_out(raw, 0) == data and tc.total(table) == len(data), name
    return Case("%s/w%d" % (name, wrapper), tc.frame(raw, data, wrapper), raw, wrapper, [tuple(t) for t in table], data, tuple(cells_))


@functools.lru_cache(maxsize=None)
def text():
    # 50 bytes: one cut at every cut_bytes; 0: empty entries (Z_SYNC_FLUSH / Z_FULL_FLUSH); 20480: a multiple of every cut_bytes
    lens = [40000, 50, 0, 0, 20480, 30000, 0, 36000, 23470]
    data = (vc.pg11() * 2)[3000:3000 + sum(lens)]
    raw, table = tc.zcut(data, lens)
    mine = ("tok_literal", "tok_match", "src_same_cut", "src_earlier_cut", "src_front_of_entry", "src_straddles_cut",
            "src_straddles_entry", "one_cut_entry", "empty_entry", "multiple_entry")
    return [_case("text", raw, table, data, w, mine if w == 0 else ()) for w in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def single():
    out = []
    data = vc.noise(150000, 61)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    out.append(_case("stored", raw, [(0, len(data))], data, 0, ("hdr_stored",)))
    data = vc.pg11()[:40000]  # (one entry behind one point: every range's lead-in begins at 0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 6, zlib.Z_FIXED)  # (memLevel 6: a block per 4096 tokens)
    raw = c.compress(data) + c.flush()
    out.append(_case("fixed", raw, [(0, len(data))], data, 0, ("tok_literal", "tok_match")))
    out.append(_case("fixed", raw, [(0, len(data))], data, 2, ()))
    return out


@functools.lru_cache(maxsize=None)
def hand():
    w = vc.BitWriter()
    table, data = [], bytearray()

    def entry(n):
        table.append((len(w.bits), n))

    def match(n, dist):
        tc.fixed_match(w, n, dist)
        for _ in range(n):
            data.append(data[-dist])

    def lits(block):
        for ch in block:
            vc.fixed_ll(w, ch)
        data.extend(block)

    def stored(block):
        w.put(0, 1).put(0, 2).align().put(len(block), 16).put(~len(block) & 0xFFFF, 16).raw(block)
        data.extend(block)

    # a header is a cut only behind a stored piece (behind a Huffman block the end-of-block token in front of it has the same
    # position): stored, a fixed block of 64 literals -- its end-of-block token is a cut at 64 --, stored, a dynamic block
    entry(20000 + 64 + 20000 + 300)
    stored(vc.noise(20000, 67))
    w.put(0, 1).put(1, 2)
    lits(vc.noise(64, 68))
    vc.fixed_ll(w, 256)
    stored(vc.noise(20000, 69))
    ll = [8] * 254 + [9] * 4  # literals, the end of the block and one length; one distance code of one bit
    vc.dynamic_header(w, ll + [1], 258, 1, bfinal=0)
    codes = vc.canonical(ll)
    for ch in vc.noise(300, 70):
        w.code(*codes[ch])
    data.extend(vc.noise(300, 70))
    w.code(*codes[256])
    # behind the point at 40000: one run of the byte in front of the entry, 12 matches of 258 -- every symbol a marker
    entry(12 * 258)
    w.put(0, 1).put(1, 2)
    for _ in range(12):
        match(258, 1)
    vc.fixed_ll(w, 256)
    # periods 7 and 13 that begin in front of the entry, then literals
    entry(4 * 258 + 4 * 258 + 100)
    w.put(0, 1).put(1, 2)
    for _ in range(4):
        match(258, 7)
    for _ in range(4):
        match(258, 13)
    lits(vc.noise(100, 71))
    vc.fixed_ll(w, 256)
    # at cut_bytes 256: a cut behind k gathered literals, k = 0 .. 63
    entry(64 * 256)
    w.put(0, 1).put(1, 2)
    for k in range(64):
        match(256 - k, 1)
        lits(vc.noise(k, 100 + k))
    vc.fixed_ll(w, 256)
    w.put(0, 1).put(0, 2).align().put(0, 16).put(0xFFFF, 16)  # an empty stored block: the next entry begins at a byte
    tail = vc.pg11()[20000:40000]
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    z = c.compress(tail) + c.flush()
    entry(len(tail))
    w.raw(z)
    data += tail
    mine = ("hdr_fixed", "hdr_dynamic", "tok_eob", "behind_258", "all_markers_3_cuts", "period_not_64", "every_lit_offset", "tok_match")
    return [_case("hand", w.bytes(), table, bytes(data), 0, mine)]


@functools.lru_cache(maxsize=None)
def corpus():
    return text() + single() + hand()


def by_name(name):
    return [c for c in corpus() if c.name == name][0]


# ---- what is read ------------------------------------------------------------------------------------------------------------------
def points(c):
    pos = tc.starts(c.table)
    pts = [0]
    for k in range(1, len(c.table)):
        if pos[k] - pos[pts[-1]] >= SPACING:
            pts.append(k)
    return pts


def ranges(c, cut_bytes, every=True):
    """[(off, len)]: ranges that begin and end at EVERY cut boundary - 1 / + 0 / + 1 of the first, a middle and the last entry behind
    the case's last point that has bytes, ranges over several entries, to the end, off >= total, len == 0.  every=False: thinned to 6
    boundaries an entry, for the forms of the host build that replay every lane or run under a sanitizer"""
    n = len(c.want)
    cl, on = cuts(c, cut_bytes)
    pts = points(c)
    behind = [e for e in range(pts[-1], len(c.table)) if c.table[e][1]]
    out = [(0, 0), (n, 10), (n + 5, 1), (0, 100), (n - 1, 1), (n - 70, 200)]
    for e in sorted({behind[0], behind[len(behind) // 2], behind[-1]}):
        mine = [x[1] for x, pl in zip(cl, on) if pl.entry == e]
        step = 1 if every else max(len(mine) // 6, 1)
        for b in mine[::step] + mine[-1:]:
            for d in (-1, 0, 1):
                if 0 <= b + d < n:
                    out.append((b + d, 1))        # begins there
                    out.append((max(b + d - 300, 0), b + d - max(b + d - 300, 0)))  # ends there
    pos = tc.starts(c.table)
    out.append((pos[pts[-1]] + 7, n))                 # to the stream's end
    out.append((max(pos[pts[-1]] - 5000, 0), 70000))  # over several entries (and a point, where there is one in front)
    return out


def batches(c, cut_bytes):
    """parts that share a set: ranges that overlap, that are the same, that decode from different points"""
    n = len(c.want)
    return [[(n // 3, 5000), (n // 3 + 2500, 5000), (n // 3, 5000), (10, 100), (n - 3000, 5000)] + [((k * 7919) % n, 50 + 37 * k) for k in range(12)]]


LONG = (1000, 150000)  # with a group budget of GROUP_MIN: a range in pieces


def flipped(stream, bit):
    m = bytearray(stream)
    m[bit >> 3] ^= 1 << (bit & 7)
    return bytes(m)


def damage(c, cut_bytes):
    """Bit flips after the build (wrapper 0), for the range (off, len) returned with them: [(kind, bit)] -- "header": in the dynamic
    header of the block that holds the range's first byte; "token": behind a middle cut of the lead-in, inside its first tokens;
    "outside": behind the range's last cut, which a read must not notice"""
    assert c.wrapper == 0
    cl, on = cuts(c, cut_bytes)
    pts = points(c)
    pos = tc.starts(c.table)
    # a dynamic block behind the last point that holds three cuts at least
    cand = collections.Counter(pl.hdr for x, pl in zip(cl, on) if pl.entry >= pts[-1] and x[0] != x[2] and c.raw[x[2] >> 3:] and
                               _bits(c.raw, x[2] + 1, 2) == 2)
    hdr = [h for h, k in sorted(cand.items()) if k >= 3][0]
    mine = [x for x in cl if x[2] == hdr]
    off, ln = mine[2][1] + 3, 40
    after = [x for x in cl if x[1] > off + ln]
    flips = [("header", hdr + 3 + k) for k in (1, 6, 20, 40)]
    flips += [("token", mine[1][0] + k) for k in (1, 9, 17, 30, 44)]
    flips += [("outside", after[0][0] + k) for k in (3, 11)] if after else []
    assert pos[pts[-1]] <= mine[0][1]
    return (off, ln), flips, hdr
