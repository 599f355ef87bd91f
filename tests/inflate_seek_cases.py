"""Cases for the seek points (include/mi355_deflate.h mi355_inflate_seek_*): seeded, shared by the CPU test of the host build
(test_inflate_seek_cases.py) and the GPU test (test_inflate_seek_gpu.py).  TEST INFRASTRUCTURE.

  (a) text()       zlib streams of text at levels 1, 6 and 9 in all three wrappers, the table the index finds for them
  (b) cut()        zlib streams cut with Z_SYNC_FLUSH into entries of 0 to 40 000 bytes -- runs of empty entries and entries shorter
                   than 32 KiB around a point --, three short entries that copy from each other, and a stream assembled bit by bit:
                   the first token behind one point is a match of distance 32768 (the window's byte 0), behind another a match of
                   distance 1 and length 258, whose source is the window's last byte
  (c) single()     stored-only and fixed-only streams: one entry, so point 0 alone
  (d) oracle()     the oracle's streams with their trace_blocks() tables
A case is a Case tuple; `want` is what zlib inflates the stream to, and the judge of a read is want[off:off + len].  Every case states
its point list for every spacing from the rule, points(); ranges() names what is read.
"""
import collections
import functools
import zlib

import inflate_table_cases as tc
import inflindex_binding as xb
import verify_cases as vc

Case = collections.namedtuple("Case", "name stream wrapper table want full")

WIN = 32768
SPACINGS = (WIN, 100000, 1 << 20)  # the smallest legal one, one between, one larger than every stream here
GROUP_DEFAULT, GROUP_MIN = tc.GROUP_DEFAULT, tc.GROUP_MIN
LENS = (0, 1, 15, 16, 17, 65536, None)  # None: to the end


def points(table, spacing):
    """the point rule: entry 0, and every entry that begins `spacing` output bytes or more behind the last point: [(bit, pos)]"""
    pos = tc.starts(table)
    pts = [0]
    for k in range(1, len(table)):
        if pos[k] - pos[pts[-1]] >= spacing:
            pts.append(k)
    return [(table[k][0], pos[k]) for k in pts]


def entry_of(table, q):
    """the entry that holds output position q"""
    pos = tc.starts(table)
    return max(k for k in range(len(table)) if pos[k] <= q and table[k][1] > 0 and q < pos[k] + table[k][1])


def decoded(table, spacing, off):
    """the entries a 1-byte read at `off` decodes: from the last point at or before it (a point is the first entry at its position)
    through the entry that holds it"""
    pos = tc.starts(table)
    p = max(q for _bit, q in points(table, spacing) if q <= off)
    return entry_of(table, off) - pos.index(p) + 1


def zcut_empty(data, lens, level=6):
    """tc.zcut with RUNS of empty entries: zlib writes no second flush block without input, so an entry of no bytes is an empty stored
    block of its own, five bytes spliced in at the cut (the cuts are byte aligned)"""
    assert sum(lens) == len(data) and lens[-1] > 0
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out, table, pos = b"", [], 0
    for k, n in enumerate(lens):
        table.append((8 * len(out), n))
        if n == 0:
            out += b"\x00\x00\x00\xff\xff"
            continue
        out += c.compress(data[pos:pos + n])
        pos += n
        out += c.flush() if k == len(lens) - 1 else c.flush(zlib.Z_SYNC_FLUSH)
    return out, table


def index_table(stream, wrapper):
    rc, _n, blocks, _spans, _rep = xb.index(stream, wrapper, xb.span_default())
    assert rc == 0
    return [(b["bit_start"], b["in_bytes"]) for b in blocks]


def text300():
    return (vc.pg11() * 3)[5000:305000]


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text():
    out = []
    data = text300()
    for level in (1, 6, 9):
        for wrapper in (0, 1, 2):
            c = zlib.compressobj(level, zlib.DEFLATED, vc.WBITS[wrapper])
            stream = c.compress(data) + c.flush()
            table = index_table(stream, wrapper)
            assert len(table) >= 3 and tc.total(table) == len(data)
            out.append(Case("text:l%d/w%d" % (level, wrapper), stream, wrapper, table, data, (level, wrapper) == (6, 0)))
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def hand_points():
    """entry 0: 32768 stored bytes; entry 1 at 32768 -- a point at spacing 32 KiB -- begins with a match of distance 32768; entry 2:
    32768 stored bytes; entry 3 at 65559 -- a point again -- begins with a match of distance 1 and length 258, then one of 32768"""
    r0, r1 = vc.noise(WIN, 31), vc.noise(WIN, 37)
    w = vc.BitWriter()
    table, data = [], bytearray()

    def stored(block, final=0):
        w.put(final, 1).put(0, 2).align().put(len(block), 16).put(~len(block) & 0xFFFF, 16).raw(block)

    table.append((len(w.bits), WIN))
    stored(r0)
    data += r0
    table.append((len(w.bits), 23))
    tc.fixed_match(w.put(0, 1).put(1, 2), 20, WIN)
    data += data[-WIN:-WIN + 20]
    for ch in b"xyz":
        vc.fixed_ll(w, ch)
    data += b"xyz"
    vc.fixed_ll(w, 256)
    table.append((len(w.bits), WIN))
    stored(r1)
    data += r1
    table.append((len(w.bits), 258 + 70))
    tc.fixed_match(w.put(1, 1).put(1, 2), 258, 1)
    data += bytes([data[-1]]) * 258
    tc.fixed_match(w, 70, WIN)
    for _ in range(70):
        data.append(data[-WIN])
    vc.fixed_ll(w, 256)
    return w.bytes(), table, bytes(data)


@functools.lru_cache(maxsize=None)
def cut():
    out = []
    txt = vc.pg11() * 3

    def add(name, raw, table, data, wrappers=(0,), full=False):
        assert tc.zlib_out(raw, 0) == data, name
        for wrapper in wrappers:
            out.append(Case("cut:%s/w%d" % (name, wrapper), tc.frame(raw, data, wrapper), wrapper, [tuple(t) for t in table], data,
                            full and wrapper == 0))

    # empty entries in front of the stream, a run of them where a point falls, entries shorter than a window around the points
    lens = [0, 40000, 0, 0, 0, 30000, 2768, 1, 20000, 12000, 0, 767, 40000, 5000, 33000, 0, 0, 31000, 1737, 40000, 38000, 10000, 0, 63]
    data = txt[7000:7000 + sum(lens)]
    raw, table = zcut_empty(data, lens)
    add("lengths", raw, table, data, wrappers=(0, 1, 2), full=True)
    # markers of markers: three short entries in a row, each a copy of the one in front of it, behind a point
    blk = vc.noise(3000, 53)
    data = txt[:40000] + blk * 4 + txt[40000:80000]
    raw, table = tc.zcut(data, [40000, 3000, 3000, 3000, 3000, 40000], level=9)
    add("copies_of_copies", raw, table, data)
    raw, table, data = hand_points()
    add("first_token_32768_and_1", raw, table, data, full=True)
    return out


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single():
    out = []
    data = vc.noise(100000, 59)
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    raw = c.compress(data) + c.flush()
    out.append(Case("single:stored/w0", raw, 0, [(0, len(data))], data, False))
    data = vc.pg11()[:100000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    raw = c.compress(data) + c.flush()
    out.append(Case("single:fixed/w0", raw, 0, [(0, len(data))], data, False))
    out.append(Case("single:fixed/w2", tc.frame(raw, data, 2), 2, [(0, len(data))], data, False))
    return out


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    names = ("oracle:pg11x3/default/w0", "oracle:pg11x3/default/w1", "oracle:pg11x3/default/w2", "oracle:pg11x3/best/w0", "oracle:pg11x3/fast/w0")
    return [Case("seek:" + c.name, c.stream, c.wrapper, [tuple(t) for t in c.table], c.want, False) for c in tc.oracle() if c.name in names]


@functools.lru_cache(maxsize=None)
def corpus():
    return text() + cut() + single() + oracle()


def by_name(name):
    return [c for c in corpus() if c.name == name][0]


# ---- what is read ------------------------------------------------------------------------------------------------------------------
def ranges(c, spacing):
    """[(off, len)]: a full case reads every off of {0, each point's pos - 1 / + 0 / + 1, an entry boundary - 1 / + 0 / + 1,
    total - 1, total, total + 5} with every len of LENS; the others a handful around their last point and their end"""
    n = len(c.want)
    pts = [p for _bit, p in points(c.table, spacing)]
    st = [p for p in tc.starts(c.table) if 0 < p < n]
    offs = {0, n - 1, n, n + 5}
    if c.full:
        for p in pts:
            offs |= {p - 1, p, p + 1}
        if st:
            e = st[len(st) // 2]
            offs |= {e - 1, e, e + 1}
        lens = LENS
    else:
        offs |= {pts[-1] - 1, pts[-1], pts[-1] + 1}
        lens = (0, 1, 17, None)
    out = []
    for off in sorted(o for o in offs if o >= 0):
        for ln in lens:
            out.append((off, max(n - off, 0) if ln is None else ln))
    return out


def alignments(c, spacing):
    """every off % 16 class with every output pointer % 8 class, around the case's last point: [(off, len, pointer class)]; 50 bytes,
    so that a range has aligned runs of 16 and a tail"""
    p = points(c.table, spacing)[-1][1]
    base = max(p - 8, 0)
    return [(base + i, 50, a) for i in range(16) for a in range(8)]


def batches(c, spacing):
    """batches of 1, 2 and 33 ranges, with ranges that overlap and ranges that are the same"""
    n = len(c.want)
    p = points(c.table, spacing)[-1][1]
    one = [(p + 5, 1000)]
    two = [(n // 3, 5000), (n // 3 + 2500, 5000)]
    many = [((k * 7919) % n, 100 + 37 * k) for k in range(30)] + [(p, 4096), (p, 4096), (n - 10, 100)]
    return [one, two, many]


LONG = (1000, 200000)  # with a group budget of GROUP_MIN: a range in pieces


def damage(c, spacing):
    """Bit flips after the build, for the range (off, len) returned with them: [(kind, bit)] -- kind "lead": in the lead-in, an entry
    in front of the one that holds off; "inside": in the entry that holds off; "behind": in the range's last entry, in its last bits,
    behind off + len; "outside": in an entry behind the range's last, which a read must not notice.  Several bits per kind: a flip may
    leave an entry that still decodes to its end."""
    pos = tc.starts(c.table)
    pts = [p for _bit, p in points(c.table, spacing)]
    # the first point that has two entries of bytes behind it and an entry behind those
    for p in pts[1:]:
        a = [k for k in range(len(c.table)) if pos[k] == p][0]
        ks = [k for k in range(a, len(c.table)) if c.table[k][1] > 0]
        if len(ks) >= 3:
            break
    else:
        raise AssertionError("no point with three entries behind it")
    k0, k1, k2 = ks[0], ks[1], ks[2]
    off, ln = pos[k1] + 10, max(c.table[k1][1] // 4, 1)
    assert c.wrapper == 0  # (a table's bits count from the first deflate byte)
    end = lambda k: c.table[k + 1][0] if k + 1 < len(c.table) else 8 * len(c.stream)  # noqa: E731
    flips = []
    for kind, k, where in (("lead", k0, (0.3, 0.5, 0.7)), ("inside", k1, (0.02, 0.05, 0.1)), ("behind", k1, (0.9, 0.95, 0.99)),
                           ("outside", k2, (0.3, 0.5, 0.7))):
        for f in where:
            flips.append((kind, c.table[k][0] + int((end(k) - c.table[k][0]) * f)))
    return (off, ln), flips


def flipped(stream, bit):
    m = bytearray(stream)
    m[bit >> 3] ^= 1 << (bit & 7)
    return bytes(m)
