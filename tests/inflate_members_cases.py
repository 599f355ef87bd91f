"""Cases for the members inflate (include/mi355_deflate.h mi355_inflate_members*): gzip FILES of one or many members, built here,
shared by the CPU test of the host build (test_inflate_members_cases.py) and the GPU test (test_inflate_members_gpu.py).
TEST INFRASTRUCTURE.

The judge of bytes, and of valid / invalid, is Python's zlib: decompressobj(31) member by member over unused_data, every member
reaching its end (zlib_members).  A case is Case(name, stream, want, caps, facts): want = zlib's bytes, or None when zlib refuses the
file; caps = out_cap values the case is run at besides its own size; facts = offsets a test asserts the case's precondition with.

  single()   the gzip frames of inflate_cases.framed() as files of one member
  plain()    sequences of ordinary members: mixed levels, every optional header field, empty members, the oracle's gzip streams
  bgzf()     members that state their size in a 'BC' subfield: block sizes, member counts, the end-of-file marker, subfield order,
             a member start at every offset mod 64
  mixed()    plain and hinted members alternating, more often than Path A resumes
  decoys()   stored payloads that look like BGZF members: shadowing a true start, linking into the true chain
  liars()    BSIZE and ISIZE that are not true
  damage()   flipped bits, truncations, trailing bytes
"""
import collections
import functools
import struct
import zlib

import inflate_cases as icases
import oracle_binding as ob
import verify_cases as vc
from verify_cases import GZ_HEADERS, gzip_frame

Case = collections.namedtuple("Case", "name stream want caps facts")

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def zlib_members(stream):
    """[the bytes of every member] as zlib inflates the file, or None if it refuses a member, a member does not reach its end, or
    the file is empty"""
    rest, out = bytes(stream), []
    if not rest:
        return None
    while rest:
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(rest))
        except zlib.error:
            return None
        if not d.eof:
            return None
        rest = d.unused_data
    return out


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gz(data, level=6, header=GZ_HEADERS["blank"]):
    """an ordinary member"""
    return gzip_frame(raw_deflate(data, level), data, header)


def bgzf(data, level=6, bsize_delta=0, isize=None, before=b"", behind=b"", bsize=None):
    """a member with a 'BC' subfield (other subfields `before` and `behind` it); bsize_delta, bsize, isize: lies"""
    raw = raw_deflate(data, level)
    xlen = len(before) + 6 + len(behind)
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536
    b = (total - 1 + bsize_delta if bsize is None else bsize) & 0xFFFF
    hdr = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + before + b"BC\x02\x00" + struct.pack("<H", b) + behind
    return hdr + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, (len(data) if isize is None else isize) & 0xFFFFFFFF)


def text(lo, n):
    t = vc.pg11()
    return (t * (1 + (lo + n) // len(t)))[lo: lo + n]


def starts(parts):
    out, o = [], 0
    for p in parts:
        out.append(o)
        o += len(p)
    return out


def case(name, parts, caps=(), **facts):
    stream = b"".join(parts)
    m = zlib_members(stream)
    facts = dict(facts, starts=starts(parts), n_parts=len(parts))
    return Case(name, stream, None if m is None else b"".join(m), tuple(caps), facts)


def boundaries(parts):
    """out_cap values around every member boundary of a valid file"""
    m = zlib_members(b"".join(parts))
    caps, p = {0, 1}, 0
    for x in m:
        p += len(x)
        caps |= {p - 1, p, p + 1}
    caps.add(p - 1)
    return sorted(c for c in caps if 0 <= c <= p + 1)


@functools.lru_cache(maxsize=None)
def single():
    return [case("single/" + name, [s]) for name, s, w in icases.framed() if w == 2]


@functools.lru_cache(maxsize=None)
def plain():
    out = []
    levels = (0, 1, 6, 9)
    for n in (2, 3, 17):
        parts = [gz(text(1000 * k, 300 + 211 * k), levels[k % 4]) for k in range(n)]
        out.append(case("plain/%d" % n, parts, boundaries(parts) if n == 3 else ()))
    parts = [gz(text(0, 500), 6, GZ_HEADERS["name"]), gz(text(500, 700), 1, GZ_HEADERS["all"]), gz(text(1200, 90), 9, GZ_HEADERS["blank"]),
             gz(vc.noise(300, 3), 6, GZ_HEADERS["all"])]
    out.append(case("plain/headers", parts))
    e, a, b = gz(b""), gz(text(0, 400)), gz(text(400, 333), 1)
    out.append(case("plain/empty_first", [e, a, b]))
    out.append(case("plain/empty_middle", [a, e, b], boundaries([a, e, b])))
    out.append(case("plain/empty_last", [a, b, e]))
    out.append(case("plain/empty_doubled", [a, e, e, b, e, e]))
    out.append(case("plain/only_empty", [e]))
    # what a packed batch encode with gzip members writes when no region needs padding: the oracle's streams back to back
    datas = [text(0, 5000), b"", text(7000, 70000), vc.noise(1000, 9), text(100, 1)]
    parts = [ob.encode_gzip(d, GZ_HEADERS["name" if k % 2 else "blank"], level=(ob.DEFAULT, ob.FAST, ob.BEST)[k % 3])
             for k, d in enumerate(datas)]
    out.append(case("plain/oracle_arena", parts))
    return out


@functools.lru_cache(maxsize=None)
def bgzf_cases():
    out = []
    sizes = (0, 1, 63, 64, 65, 0xff00)
    parts = [bgzf(text(17 * n, n) if n < 0xff00 else vc.noise(n, 21), 6 if n < 0xff00 else 1) for n in sizes] + [BGZF_EOF]
    out.append(case("bgzf/blocks", parts, boundaries(parts)))
    for n in (1, 2, 65, 130):
        parts = [bgzf(text(90 * k, 40 + (k * 7) % 50), (1, 6, 9)[k % 3]) for k in range(n)]
        out.append(case("bgzf/n%d" % n, parts))
    a, b, c = bgzf(text(0, 3000)), bgzf(text(3000, 2000), 1), bgzf(vc.noise(500, 4))
    out.append(case("bgzf/eof_last", [a, b, c, BGZF_EOF], boundaries([a, b, c, BGZF_EOF])))
    out.append(case("bgzf/eof_middle", [a, BGZF_EOF, b, c]))
    out.append(case("bgzf/eof_doubled", [a, b, BGZF_EOF, BGZF_EOF]))
    out.append(case("bgzf/only_eof", [BGZF_EOF]))
    out.append(case("bgzf/bc_behind_a_subfield", [bgzf(text(0, 700), before=b"AB\x03\x00xyz"), bgzf(text(700, 100), before=b"BC\x01\x00q")]))
    out.append(case("bgzf/bc_in_front_of_a_subfield", [bgzf(text(0, 700), behind=b"ZZ\x00\x00"), bgzf(text(700, 100), behind=b"BC\x02\x00\x01\x00")]))
    # member starts on every offset mod 64 (and so mod 16), the first on a span edge: the sizes of the members walk the residues
    parts, seen, k = [], set(), 0
    while len(seen) < 64 and k < 2000:
        seen.add(sum(map(len, parts)) % 64)
        parts.append(bgzf(vc.noise(20 + k % 37, 100 + k), 0))
        k += 1
    out.append(case("bgzf/every_residue", parts))
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    p = [gz(text(50 * k, 200 + k), (1, 6)[k % 2]) for k in range(12)]
    h = [bgzf(text(3000 + 80 * k, 150 + k), (6, 9)[k % 2]) for k in range(24)]
    out = [case("mixed/plain_then_hinted", p[:2] + h[:5]),
           case("mixed/hinted_plain_hinted", h[:3] + p[:2] + h[3:7], boundaries(h[:3] + p[:2] + h[3:7]))]
    parts = []
    for k in range(11):  # more alternations than Path A resumes: the tail is walked by Path B with the hints ignored
        parts += [p[k], h[2 * k], h[2 * k + 1]]
    out.append(case("mixed/alternating_11", parts, alternations=11))
    return out


def stored_member(payload):
    assert len(payload) <= 65535
    return gz(payload, 0)


@functools.lru_cache(maxsize=None)
def decoys():
    out = []
    inner = b"".join([bgzf(text(0, 300)), bgzf(text(300, 200), 1), BGZF_EOF])
    h = [bgzf(text(1000 + 100 * k, 120 + k)) for k in range(6)]
    out.append(case("decoy/stored_bgzf_file", h[:2] + [stored_member(inner)] + h[2:], inner=len(inner)))
    # a hinted header inside the stored payload of a hinted member, in front of a true start in the same span of 64 bytes: it
    # shadows the true start
    for n0 in range(60, 200):
        h0 = bgzf(vc.noise(n0, 5), 0)
        d = len(h0) + 23  # the carrying member's 18 header bytes and the 5 of its stored block
        if d // 64 >= 1 and d % 64 < 38:
            break
    fake = bgzf(b"", bsize=29)[:18]  # claims 30 bytes: it ends inside the true member behind it, where nothing is hinted
    h1 = bgzf(text(0, 500))
    out.append(case("decoy/shadow", [h0, bgzf(fake, 0), h1, h[0], h[1]], decoy=d, true=d + 18 + 8))
    # ... and one whose claimed extent ends exactly on a later true start that is its span's candidate
    L = 150
    fake = (bgzf(b"", bsize=L + 8 - 1)[:18]).ljust(L, b"\0")
    out.append(case("decoy/lands_on_a_true_start", [h0, bgzf(fake, 0), h1, h[0], h[1]], decoy=d, true=d + L + 8))
    return out


@functools.lru_cache(maxsize=None)
def liars():
    out = []
    d = [text(500 * k, 400 + 10 * k) for k in range(5)]
    good = [bgzf(x) for x in d]
    for delta in (1, -1):
        parts = good[:2] + [bgzf(d[2], bsize_delta=delta)] + good[3:]
        out.append(case("liar/bsize%+d" % delta, parts))
    out.append(case("liar/bsize_past_the_end", good[:4] + [bgzf(d[4], bsize_delta=100)]))
    out.append(case("liar/bsize_first_member", [bgzf(d[0], bsize_delta=-1)] + good[1:]))
    two = len(good[1]) + len(good[2])
    out.append(case("liar/bsize_spans_two_members", [good[0], bgzf(d[1], bsize=two - 1)] + good[2:]))
    at = len(d[0]) + len(d[1]) + len(d[2])  # where the lying member's output ends
    total = sum(map(len, d))
    caps = sorted({total + 1, total, total - 1, at + 1, at, at - 1, at - len(d[2]), at + 7, at - 7})
    for name, lie in (("small", len(d[2]) - 7), ("large", len(d[2]) + 7)):
        out.append(case("liar/isize_too_%s" % name, good[:2] + [bgzf(d[2], isize=lie)] + good[3:], caps, at=at, total=total))
    out.append(case("liar/isize_plain_member", [gz(d[0]), gzip_frame(raw_deflate(d[1]), d[1] + b"x", GZ_HEADERS["blank"]), gz(d[2])],
                    (len(d[0]) + len(d[1]) - 1, len(d[0]) + len(d[1]), total)))
    return out


def flip(stream, byte, bit=0):
    s = bytearray(stream)
    s[byte] ^= 1 << bit
    return bytes(s)


@functools.lru_cache(maxsize=None)
def damage():
    out = []
    d = [text(700 * k, 600 + k) for k in range(5)]
    for kind, parts in (("bgzf", [bgzf(x) for x in d]), ("plain", [gz(x, 6, GZ_HEADERS["name"]) for x in d])):
        whole = b"".join(parts)
        st = starts(parts)
        hdr = 18 if kind == "bgzf" else len(GZ_HEADERS["name"])
        for which, k in (("first", 0), ("middle", 2), ("last", 4)):
            o, n = st[k], len(parts[k])
            for part, byte, bit in (("magic", o, 2), ("cm", o + 2, 0), ("data", o + hdr + (n - hdr - 8) // 2, 3), ("data0", o + hdr, 1),
                                    ("crc", o + n - 8, 0), ("isize", o + n - 4, 0)):
                out.append(case("damage/%s/%s/%s" % (kind, which, part), [flip(whole, byte, bit)], damaged=k))
        o, n = st[4], len(parts[4])
        for part, cut in (("header", o + 5), ("data", o + hdr + 20), ("trailer", o + n - 3), ("member_edge", o), ("second_header", st[1] + 11)):
            out.append(case("damage/%s/cut_in_%s" % (kind, part), [whole[:cut]]))
        out.append(case("damage/%s/trailing_zeros" % kind, [whole + bytes(16)]))
        out.append(case("damage/%s/one_trailing_byte" % kind, [whole + b"\x1f"]))
    if True:  # a BSIZE field damaged: the file stays valid, the hint is what lies
        parts = [bgzf(x) for x in d]
        whole = b"".join(parts)
        out.append(case("damage/bgzf/bsize_field", [flip(whole, starts(parts)[2] + 16, 0)]))
    out.append(case("damage/empty_file", [b""]))
    out.append(case("damage/seventeen_bytes", [gz(b"")[:17]]))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    out = single() + plain() + bgzf_cases() + mixed() + decoys() + liars() + damage()
    assert len({c.name for c in out}) == len(out)
    assert sum(len(c.stream) for c in out) < 4 << 20
    return out


def by_name(name):
    return next(c for c in corpus() if c.name == name)
