"""Cases for the large plain members of the members inflate (include/mi355_deflate.h mi355_inflate_members*,
MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES): gzip FILES whose members state no size and are large enough to be found and decoded in
parallel, built here, shared by the CPU test of the host build (test_inflate_bigmembers_cases.py) and the GPU test
(test_inflate_bigmembers_gpu.py).  TEST INFRASTRUCTURE.

Every case is meant for the threshold THRESHOLD = 1 KiB and runs at the index spans SPANS = 256 and 4096 bytes.  The judge of bytes,
and of valid / invalid, is Python's zlib (inflate_members_cases.zlib_members).  A case is Case(name, stream, want, caps, expect, facts):
want = zlib's bytes, or None when zlib refuses the file; caps = out_cap values besides the case's own size; expect = the members the
parallel path decodes on a valid file (expected_parallel, the rule of DESIGN.md section 15 written out over the member list; None
for a refused file); facts = what a test asserts the case's precondition with.

  valid()    2, 3 and 5 members; a start at every offset mod 8; first blocks that are and are not a candidate; an empty and a
             30-byte member between large ones; stored-only and one-fixed-block members; BGZF runs around a large plain member; a
             packed gzip arena; a member over three groups of 64 KiB and a group over three members; a BFINAL block that ends on a
             byte boundary and inside a byte; ends and boundaries at an extent's edge and one bit behind it; a decoy header inside a
             stored block at a span's start
  damage()   flipped bits in a dynamic header and in a symbol, a distance into the member in front, wrong CRC and ISIZE, truncations,
             trailing bytes -- in the first, a middle and the last member
  short()    out_cap at every member boundary +- 1, inside an entry, 0
"""
import collections
import functools
import struct
import zlib

import datagen
import inflate_members_cases as mc
import oracle_binding as ob
from verify_cases import GZ_HEADERS, gzip_frame

Case = collections.namedtuple("Case", "name stream want caps expect facts")

THRESHOLD = 1024
SPANS = (256, 4096)
GROUP_SMALL = 64 << 10
RESUMES = 8  # Path A resumes of one call (inflate_members.h)


@functools.lru_cache(maxsize=None)
def _text():
    return bytes(datagen.text_like(1 << 20, 20250101))


def text(lo, n):
    t = _text()
    assert lo + n <= len(t)
    return t[lo: lo + n]


def named_header(k):
    """a gzip header of 11 + k bytes (FNAME of k - 1 characters), k >= 1"""
    return bytes([0x1f, 0x8b, 8, 8, 0, 0, 0, 0, 0, 0xff]) + b"n" * (k - 1) + b"\0"


# ---- deflate by hand: the blocks zlib does not write on request -------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):  # k bits, least significant first
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code, most significant bit first
        self.put(int(format(c, "0%db" % k)[::-1], 2), k)

    def bits(self):
        return 8 * len(self.out) + self.n

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def stored(self, data, final=0):
        assert len(data) <= 65535
        self.put(final, 1)
        self.put(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data)

    def fixed_lit(self, v):
        if v < 144:
            self.code(0x30 + v, 8)
        else:
            self.code(0x190 + v - 144, 9)

    def fixed(self, lits, final=0, match=None):
        """a fixed block of literals; match = (3, dist in 97 .. 128) behind them"""
        self.put(final, 1)
        self.put(1, 2)
        for v in lits:
            self.fixed_lit(v)
        if match:
            assert match[0] == 3 and 97 <= match[1] <= 128
            self.code(1, 7)   # length symbol 257: 3
            self.code(13, 5)  # distance symbol 13: 97 .. 128, five extra bits
            self.put(match[1] - 97, 5)
        self.code(0, 7)

    def raw(self, deflate):
        """a whole raw deflate stream behind a byte boundary"""
        assert self.n == 0
        self.out += deflate

    def done(self):
        assert self.n == 0
        return bytes(self.out)


def member(raw, data, header=GZ_HEADERS["blank"]):
    return gzip_frame(raw, data, header)


def expected_parallel(lens, hinted, T=THRESHOLD):
    """The members of a VALID file that the parallel path decodes.  Path A takes every run of hinted members.  Path B's launch at
    member i: with fewer than T bytes left the one wave walks on to the next hinted header or the file's end; else members are
    discovered one after the other -- each is decoded in parallel -- until a hinted header follows, a member shorter than T has been
    found (the one wave takes the rest of the launch), fewer than T bytes are left (likewise) or the file ends."""
    n, i, par, resumes = len(lens), 0, 0, 0
    left = [sum(lens[k:]) for k in range(n + 1)]
    path_a = True
    while i < n:
        if path_a:
            path_a = False
            while i < n and hinted[i]:
                i += 1
            continue
        ignore = resumes >= RESUMES
        count, serial = 0, left[i] < T
        while i < n:
            if count and hinted[i] and not ignore:
                break
            if not serial and left[i] < T:
                serial = True
            if not serial:
                par += 1
                serial = lens[i] < T
            i += 1
            count += 1
        if i < n:
            resumes += 1
            path_a = True
    return par


def case(name, parts, caps=(), hinted=None, **facts):
    stream = b"".join(parts)
    m = mc.zlib_members(stream)
    facts = dict(facts, starts=mc.starts(parts), n_parts=len(parts))
    expect = None
    if m is not None:
        assert len(m) == len(parts), name
        expect = expected_parallel([len(p) for p in parts], hinted or [False] * len(parts))
    return Case(name, stream, None if m is None else b"".join(m), tuple(caps), expect, facts)


def big(k, n, level):
    """large plain member number k: n bytes of text"""
    return mc.gz(text(37000 * k, n), level)


# ---- the members with a shape --------------------------------------------------------------------------------------------------------
def first_stored(data):
    w = Bits()
    w.stored(data[:1500])
    w.raw(mc.raw_deflate(data[1500:], 6))
    return member(w.done(), data)


def first_fixed(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    head = c.compress(data[:1500]) + c.flush(zlib.Z_FULL_FLUSH)  # fixed blocks, then an empty stored one: a byte boundary
    return member(head + mc.raw_deflate(data[1500:], 6), data)


def one_fixed_block(data):
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    return member(c.compress(data) + c.flush(), data)


def ends_on_a_byte(data):
    """the BFINAL block is fixed, six 9-bit literals: 3 + 54 + 7 bits behind a byte boundary"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    w = Bits()
    w.raw(c.compress(data) + c.flush(zlib.Z_FULL_FLUSH))
    tail = bytes([200, 201, 202, 203, 204, 205])
    w.fixed(tail, final=1)
    assert w.n == 0
    return member(w.done(), data + tail)


def ends_inside_a_byte(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    w = Bits()
    w.raw(c.compress(data) + c.flush(zlib.Z_FULL_FLUSH))
    w.fixed(b"a", final=1)  # 18 bits
    assert w.n == 2
    w.align()
    return member(w.done(), data + b"a")


def edge_member(S, kind, data):
    """A member whose deflate data meets the edge of the first extent -- bit 8 E S, E = THRESHOLD / S spans, one at least -- with
    kind = 'boundary0' / 'boundary1': a block boundary that is not the last at the edge / one bit behind it (the extent must grow);
    'final0' / 'final1': the BFINAL block ends there"""
    edge = max(THRESHOLD // S, 1) * S  # bytes
    w = Bits()
    if kind == "final0":
        w.stored(data[:edge - 10 - 7])
        w.stored(data[edge - 17: edge - 10], final=1)
        used = edge - 10
    elif kind == "boundary0":
        w.stored(data[:edge - 5])
        used = edge - 5
    else:  # three empty fixed blocks and one of a 9-bit literal: 49 bits from the byte edge - 6
        w.stored(data[:edge - 11])
        for _ in range(3):
            w.fixed(b"")
        w.fixed(bytes([222]), final=1 if kind == "final1" else 0)
        used = edge - 11
        data = data[:used] + bytes([222]) + data[used:]
        used += 1
    at = w.bits()
    if kind.startswith("boundary"):
        w.stored(data[used: used + 100])  # (its header pads to a byte boundary)
        w.raw(mc.raw_deflate(data[used + 100:], 6))
    else:
        w.align()
        data = data[:used]
    assert at == 8 * edge + (1 if kind.endswith("1") else 0), (kind, at, edge)
    return member(w.done(), data)


def decoy_member(S, data, k=2):
    """a stored block whose payload begins at the start of span k and is the head of a real non-final dynamic block; the member's next
    true block begins in the same span, behind the decoy"""
    real = mc.raw_deflate(text(500000, 200000), 6)
    assert real[0] & 7 == 4  # BFINAL 0, BTYPE 2
    w = Bits()
    w.stored(data[:k * S - 10])
    w.stored(real[:120])
    assert len(w.out) == k * S + 120
    w.raw(mc.raw_deflate(data[k * S - 10:], 6))
    return member(w.done(), data[:k * S - 10] + real[:120] + data[k * S - 10:])


def far_distance_member(data):
    """a fixed block of one literal and a match 100 bytes back -- into the member in front, if there is one -- then valid blocks"""
    w = Bits()
    w.fixed(b"a", match=(3, 100))
    w.stored(b"")
    w.raw(mc.raw_deflate(data, 6))
    return member(w.done(), b"a???" + data)  # (what the trailer says does not matter: the member is refused)


@functools.lru_cache(maxsize=None)
def valid():
    out = []
    levels = (1, 6, 9)
    for n in (2, 3, 5):
        parts = [big(k, 20000 + 9000 * k, levels[k % 3]) for k in range(n)]
        out.append(case("valid/plain%d" % n, parts))
    out.append(case("valid/plain_300k", [big(0, 300000, 6), big(1, 25000, 1)]))
    # a start at every offset mod 8: the header's name makes up the residue
    parts = []
    for k in range(9):
        want = (k + 1) % 8
        for pad in range(1, 9):
            p = mc.gz(text(21000 * k, 20000 + 13 * k), levels[k % 3], named_header(pad))
            if (sum(map(len, parts)) + len(p)) % 8 == want:
                break
        parts.append(p)
    assert {o % 8 for o in mc.starts(parts)} == set(range(8))
    out.append(case("valid/every_offset_mod_8", parts))
    a, b, c = big(0, 24000, 6), big(1, 30000, 9), big(2, 21000, 1)
    out.append(case("valid/first_block_stored", [a, first_stored(text(100000, 26000)), b]))
    out.append(case("valid/first_block_fixed", [a, first_fixed(text(100000, 26000)), b]))
    e, tiny = mc.gz(b""), mc.gz(b"x" * 7, 0)
    assert len(tiny) == 30
    out.append(case("valid/empty_between", [a, e, b], small=1))
    out.append(case("valid/tiny_between", [a, tiny, b], small=1))
    out.append(case("valid/stored_only", [a, mc.gz(text(200000, 150000), 0), b]))
    out.append(case("valid/one_fixed_block", [a, one_fixed_block(text(200000, 20000)), b]))
    h = [mc.bgzf(text(3000 + 800 * k, 1500 + k), (6, 9)[k % 2]) for k in range(8)]
    out.append(case("valid/bgzf_plain_bgzf", h[:4] + [b] + h[4:], hinted=[True] * 4 + [False] + [True] * 4))
    out.append(case("valid/bgzf_two_plain_bgzf_plain", h[:2] + [a, b] + h[2:5] + [c], hinted=[True] * 2 + [False] * 2 + [True] * 3 + [False]))
    # what the packed batch encode writes with gzip members at align 4 when every item's length is a multiple of 4: back to back
    parts = []
    for k, n in enumerate((30000, 20000, 26000, 22000)):
        for pad in range(1, 5):
            p = ob.encode_gzip(text(60000 * k, n), named_header(pad), level=(ob.DEFAULT, ob.FAST, ob.BEST)[k % 3])
            if len(p) % 4 == 0:
                break
        assert len(p) % 4 == 0
        parts.append(p)
    out.append(case("valid/packed_arena", parts))
    out.append(case("valid/three_groups", [big(3, 260000, 6), a]))
    out.append(case("valid/group_of_three", [big(k, 20000, 6) for k in range(3)]))
    # (the members around the one in question end inside a byte by construction, whatever zlib's own do)
    m0, m2 = ends_inside_a_byte(text(330000, 21000)), ends_inside_a_byte(text(360000, 23000))
    out.append(case("valid/ends_on_a_byte", [m0, ends_on_a_byte(text(300000, 22000)), m2]))
    out.append(case("valid/ends_inside_a_byte", [m0, ends_inside_a_byte(text(300000, 22000)), m2]))
    for S in SPANS:
        for kind in ("final0", "final1", "boundary0", "boundary1"):
            out.append(case("valid/edge/%d/%s" % (S, kind), [a, edge_member(S, kind, text(400000, 30000)), c], span=S))
        # a decoy in the member in the middle, inside its first extents; and one in the first and in the last member, in a span that a
        # member's first extent of THRESHOLD / S spans does not hold: the finder meets it after the extent has grown
        far = max(THRESHOLD // S, 1) + 2
        out.append(case("valid/decoy/%d/middle" % S, [a, decoy_member(S, text(400000, 30000)), c], span=S, decoy_span=2))
        out.append(case("valid/decoy/%d/first" % S, [decoy_member(S, text(400000, 30000), far), a, c], span=S, decoy_span=far))
        out.append(case("valid/decoy/%d/last" % S, [a, c, decoy_member(S, text(400000, 30000), far)], span=S, decoy_span=far))
    return out


def flip(stream, byte, bit=0):
    s = bytearray(stream)
    s[byte] ^= 1 << bit
    return bytes(s)


@functools.lru_cache(maxsize=None)
def damage():
    out = []
    d = [text(50000 * k, 22000 + 1000 * k) for k in range(3)]
    parts = [mc.gz(x, 6) for x in d]
    whole, st = b"".join(parts), mc.starts(parts)
    for which, k in (("first", 0), ("middle", 1), ("last", 2)):
        o, n = st[k], len(parts[k])
        for what, byte, bit in (("dynamic_header", o + 10 + 1, 5), ("symbol", o + 10 + n // 2, 3), ("crc", o + n - 8, 0), ("isize", o + n - 4, 0)):
            out.append(case("damage/%s/%s" % (which, what), [flip(whole, byte, bit)], damaged=k))
        far = far_distance_member(d[k])
        out.append(case("damage/%s/far_distance" % which, parts[:k] + [far] + parts[k + 1:], damaged=k))
        out.append(case("damage/%s/cut_in_blocks" % which, [whole[:o + n // 2]], damaged=k))
        out.append(case("damage/%s/cut_in_trailer" % which, [whole[:o + n - 3]], damaged=k))
        if k < 2:
            out.append(case("damage/%s/cut_in_next_header" % which, [whole[:o + n + 5]], damaged=k + 1))
    out.append(case("damage/trailing_zeros", [whole + bytes(16)], damaged=3))
    out.append(case("damage/trailing_noise", [whole + bytes(range(256)) * 8], damaged=3))
    return out


@functools.lru_cache(maxsize=None)
def short():
    parts = [big(k, 21000 + 500 * k, (6, 1, 9)[k]) for k in range(3)]
    caps = set(mc.boundaries(parts)) | {10000, 21000 + 11111}
    return [case("short/plain3", parts, sorted(caps))]


@functools.lru_cache(maxsize=None)
def corpus():
    out = valid() + damage() + short()
    assert len({c.name for c in out}) == len(out)
    assert all(c.want is not None for c in valid() + short()) and all(c.want is None for c in damage())
    assert sum(len(c.stream) for c in out) < 4 << 20
    return out


def by_name(name):
    return next(c for c in corpus() if c.name == name)
