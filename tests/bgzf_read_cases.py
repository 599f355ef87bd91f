"""Cases for the BGZF reads (include/mi355_deflate.h mi355_bgzf_index_*, mi355_bgzf_read*), shared by the CPU test of the host build
(test_bgzf_read_cases.py) and the GPU test (test_bgzf_read_gpu.py).  TEST INFRASTRUCTURE.

Files come from the builders that exist: inflate_members_cases.bgzf(...) with its lies, and bgzf_cases.model(...) for the library's own
files.  The judge is Python's zlib: the bytes of every member (zlib_table), and whether a damaged member still inflates
(member_fails).  A case is Case(name, file, read_file, index, ranges, aligns, budget, expect):
  file       what the index is made from -- index "build": from the file's own claims, "members": from zlib's table of it
  read_file  what the reads decode from: the file, or a damaged copy of the same length
  ranges     [(off, len)], run as ONE batch and each alone
  aligns     per range the class mod 16 of its buffer's address, or None
  budget     the scratch of a launch set
  expect     {range index: (kind, member)} for the ranges that must fail: kind "FRAME", "TABLE", "CHECKSUM" with out_pos = the member's
             out_off, or "ANY": a failure of the member's own inside it; every other range must succeed with the bytes of image(case)
"""
import collections
import functools
import struct
import zlib

import bgzf_cases as bc
import inflate_members_cases as imc

Case = collections.namedtuple("Case", "name file read_file index ranges aligns budget expect")

GROUP_DEFAULT = 256 << 20
GROUP_MIN = 64 << 10
SET_MEMBERS = 16384


def zlib_table(file):
    """[(in_off, in_len, out_off, bytes)] of the members as zlib inflates the file"""
    rows, o, p = [], 0, 0
    while o < len(file):
        d = zlib.decompressobj(31)
        data = d.decompress(file[o:])
        assert d.eof
        n = len(file) - o - len(d.unused_data)
        rows.append((o, n, p, data))
        o += n
        p += len(data)
    return rows


def claims(file):
    """[(in_off, in_len, out_off, out_len)] as the file's own BSIZE and ISIZE fields claim them"""
    rows, o, p = [], 0, 0
    while o < len(file):
        n = struct.unpack_from("<H", file, o + 16)[0] + 1
        isize = struct.unpack_from("<I", file, o + n - 4)[0]
        rows.append((o, n, p, isize))
        o += n
        p += isize
    assert o == len(file)
    return rows


def true_members(file):
    """[the bytes of every member] of a BGZF file whose BSIZEs are true, whatever its trailers say"""
    out = []
    for o, n, _p, _z in claims(file):
        xlen = struct.unpack_from("<H", file, o + 10)[0]
        d = zlib.decompressobj(-15)
        out.append(d.decompress(file[o + 12 + xlen:o + n - 8]))
        assert d.eof and not d.unused_data
    return out


def claimed_prefix(file):
    """the sum of the ISIZEs of the members a walk by BSIZE from byte 0 hops over, until a byte that begins no such member"""
    o = p = 0
    while o < len(file):
        if len(file) - o < 18 or file[o:o + 3] != b"\x1f\x8b\x08" or file[o + 3] & 0xE4 != 4 or file[o + 12:o + 16] != b"BC\x02\x00":
            break
        n = struct.unpack_from("<H", file, o + 16)[0] + 1
        if n > len(file) - o or n < 26:
            break
        p += struct.unpack_from("<I", file, o + n - 4)[0]
        o += n
    return p


def table(case):
    """the member table the case's index must hold: [(in_off, in_len, out_off, out_len)]"""
    if case.index == "members":
        return [(o, n, p, len(d)) for o, n, p, d in zlib_table(case.file)]
    return claims(case.file)


def image(case):
    """the uncompressed bytes as the index lays them out: every member's true bytes cut or padded to its claim (they are the file's
    bytes wherever the claims are true)"""
    return b"".join(d[:t[3]].ljust(t[3], b"?") for d, t in zip(true_members(case.file), table(case)))


def member_fails(file, in_off, in_len):
    """does zlib refuse file[in_off, in_off + in_len) as one gzip member?"""
    d = zlib.decompressobj(31)
    try:
        d.decompress(file[in_off:in_off + in_len])
    except zlib.error:
        return True
    return not d.eof or bool(d.unused_data)


def touched(tab, off, length):
    """the members range (off, len) touches: their intervals intersect, empty ones never"""
    total = tab[-1][2] + tab[-1][3]
    got = 0 if off >= total else min(length, total - off)
    return [k for k, (_o, _n, p, z) in enumerate(tab) if z and got and p < off + got and off < p + z]


def plan_counts(tab, ranges, budget):
    """the plan's counts, from its definition: (distinct, in_place, scratch, pieces, sets)"""
    total = tab[-1][2] + tab[-1][3]
    wants = collections.defaultdict(list)
    for off, length in ranges:
        got = 0 if off >= total else min(length, total - off)
        for k in touched(tab, off, length):
            wants[k].append(off <= tab[k][2] and off + got >= tab[k][2] + tab[k][3])
    in_place = scratch = pieces = sets = 0
    members_in_set = bytes_in_set = None
    for k in sorted(wants):
        place = len(wants[k]) == 1 and wants[k][0]
        need = 0 if place else (tab[k][3] + 15) // 16 * 16
        assert need <= budget
        if members_in_set is None or members_in_set >= SET_MEMBERS or bytes_in_set + need > budget:
            sets, members_in_set, bytes_in_set = sets + 1, 0, 0
        members_in_set += 1
        bytes_in_set += need
        in_place += place
        scratch += not place
        pieces += 0 if place else len(wants[k])
    return dict(distinct=len(wants), in_place=in_place, scratch=scratch, pieces=pieces, sets=sets)


def case(name, file, ranges, read_file=None, index="build", aligns=None, budget=GROUP_DEFAULT, expect=None):
    assert read_file is None or len(read_file) == len(file)
    assert aligns is None or len(aligns) == len(ranges)
    return Case(name, bytes(file), bytes(file if read_file is None else read_file), index, tuple(ranges), None if aligns is None else tuple(aligns),
                budget, dict(expect or {}))


# ---- the files ------------------------------------------------------------------------------------------------------------------
SMALL_LENS = (0, 17, 0, 0, 32, 1, 200, 0, 48, 2, 163, 19, 0, 100, 36, 5, 21, 70, 0, 199, 54, 7, 88, 0, 0, 137, 9, 122, 171, 10, 44, 0, 75, 13,
              30, 93, 15, 16, 182, 0)


@functools.lru_cache(maxsize=None)
def small_parts():
    """40 members of out_len 0 to 200: every length mod 16, empty members first, doubled, between full ones and last"""
    assert {n % 16 for n in SMALL_LENS if n} == set(range(16)) and len(SMALL_LENS) == 40 and max(SMALL_LENS) == 200
    parts, lo = [], 0
    for k, n in enumerate(SMALL_LENS):
        parts.append(imc.bgzf(imc.text(lo, n), (1, 6, 9, 0)[k % 4]) if n else imc.BGZF_EOF)
        lo += n
    return tuple(parts)


@functools.lru_cache(maxsize=None)
def small_file():
    return b"".join(small_parts())


@functools.lru_cache(maxsize=None)
def big_file():
    """a member of 65280 bytes between small ones"""
    return b"".join([imc.bgzf(imc.text(0, 300)), imc.bgzf(imc.text(300, 65280), 1), imc.bgzf(imc.text(70000, 700), 9), imc.BGZF_EOF])


@functools.lru_cache(maxsize=None)
def model_file():
    """the library's own file, as the header defines it: 1000 bytes of text in blocks of 64"""
    return bc.model(imc.text(0, 1000), "default", 64)[0]


def starts_lens(file):
    return [(p, z) for _o, _n, p, z in claims(file)]


# ---- the ranges -----------------------------------------------------------------------------------------------------------------
def residues():
    """ranges that begin and end on every residue of a member, for members of 1, 2, 5, 16, 17 and 21 bytes"""
    out = []
    sl = starts_lens(small_file())
    for z in (1, 2, 5, 16, 17, 21):
        p = next(p for p, zz in sl if zz == z)
        ranges = [(p + a, b - a) for a in range(z) for b in range(a + 1, z + 1)]
        out.append(case("residues/len%d" % z, small_file(), ranges))
    return out


def boundaries():
    """one byte around every member boundary, and the end of the file"""
    sl = starts_lens(small_file())
    total = sl[-1][0] + sl[-1][1]
    ranges = []
    for p in sorted({p for p, _z in sl} | {total}):
        for a, n in ((p - 1, 1), (p - 1, 2), (p, 1), (p - 2, 4), (p - 1, 3)):
            if a >= 0:
                ranges.append((a, n))
    ranges += [(total - 1, 1), (total - 1, 100), (total - 5, 5), (total - 5, 6)]
    return [case("boundaries", small_file(), ranges)]


def alignments():
    """out pointers at every % 16 against sources at every % 16, piece lengths 0 to 48"""
    p, z = next((p, z) for p, z in starts_lens(small_file()) if z == 200)
    ranges, aligns = [], []
    for d in range(16):
        for s in range(16):
            j = d * 16 + s
            for n in (1 + j % 48, 48 - j % 16):
                ranges.append((p + s, n))
                aligns.append(d)
    for d in (0, 7):
        ranges.append((p + 3, 0))
        aligns.append(d)
    return [case("alignments", small_file(), ranges, aligns=aligns)]


def spans():
    sl = [(p, z) for p, z in starts_lens(small_file()) if z]
    total = sl[-1][0] + sl[-1][1]
    p1, z1 = sl[3]
    ranges = [(p1 + 1, z1 - 2),                                   # wholly inside one member
              (p1, z1),                                           # exactly one member: in place
              (p1, z1 + sl[4][1]),                                # exactly two
              (p1 + 2, z1 + sl[4][1] + sl[5][1] - 3),             # cuts three
              (sl[6][0] - 1, sl[6][1] + sl[7][1] + 2),            # two in place between two cut ones
              (0, total), (0, total + 50), (1, total - 2),        # all members
              (total, 10), (total + 1000, 3), (1 << 62, 1 << 62), # off >= total
              (5, 0), (total, 0)]                                 # len = 0
    out = [case("spans/small", small_file(), ranges), case("spans/small/from_members", small_file(), ranges, index="members")]
    t = len(imc.text(0, 1000))
    out.append(case("spans/model", model_file(), [(0, t), (63, 2), (64, 64), (100, 500), (999, 1), (1000, 1), (3, 0)]))
    out.append(case("spans/big", big_file(), [(0, 300 + 65280 + 700), (300, 65280), (299, 2), (300 + 65279, 2), (1000, 50000)]))
    return out


def shared():
    """batches in which ranges share members"""
    sl = [(p, z) for p, z in starts_lens(small_file()) if z]
    (pa, za), (pb, zb), (pc, zc) = sl[5], sl[6], sl[7]
    return [
        # one range covers member b, another only cuts it: b goes to scratch with two pieces; a and c are cut by one range each
        case("shared/covered_and_cut", small_file(), [(pb, zb), (pb + 3, 5)]),
        case("shared/cut_and_covered", small_file(), [(pb + 3, 5), (pb - 1, zb + 2)]),
        # three ranges inside one member, two of them the same range
        case("shared/three_in_one", small_file(), [(pb + 1, 4), (pb + 1, 4), (pb, zb)]),
        # the same whole member twice: shared, so scratch
        case("shared/whole_twice", small_file(), [(pb, zb), (pb, zb)]),
        # overlapping ranges over three members, in no order
        case("shared/overlapping", small_file(), [(pb + 1, zb + zc - 2), (pa, za + zb), (pc, zc), (pa + za - 1, 2)]),
    ]


def budgets():
    """launch sets cut by a scratch budget of 64 KiB"""
    f = big_file()
    return [
        case("budget/three_sets", f, [(10, 5), (400, 100), (300 + 65280 + 5, 20)], budget=GROUP_MIN),
        case("budget/two_sets", f, [(10, 5), (300 + 65280 + 5, 20), (400, 100), (11, 2)], budget=66000),
        case("budget/big_alone", f, [(301, 65278)], budget=GROUP_MIN),
        case("budget/big_in_place", f, [(290, 65280 + 20)], budget=GROUP_MIN),
        case("budget/small", small_file(), [(1, sum(SMALL_LENS) - 2), (3, 400)], budget=GROUP_MIN),
    ]


# ---- damage -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damage_parts():
    d = [imc.text(700 * k, 600 + k) for k in range(5)]
    return tuple(d), tuple(imc.bgzf(x) for x in d) + (imc.BGZF_EOF,)


def damage():
    d, parts = damage_parts()
    whole = b"".join(parts)
    st = imc.starts(parts)
    outs = [sum(map(len, d[:k])) for k in range(5)]
    out = []
    # the ranges: one that touches members 1, 2 and 3 with both ends cut, one inside member 0, one that covers member 4
    ranges = [(outs[1] + 10, outs[3] + 20 - outs[1] - 10), (5, 100), (outs[4], len(d[4]))]
    hit = {0: [1], 1: [0], 2: [0], 3: [0], 4: [2]}  # member -> the ranges that touch it
    for k in range(5):
        o, n = st[k], len(parts[k])
        for part, byte, bit, kind in (("magic", o, 2, "FRAME"), ("cm", o + 2, 0, "FRAME"), ("data", o + 18 + (n - 26) // 2, 3, "ANY"),
                                      ("data0", o + 18, 1, "ANY"), ("crc", o + n - 8, 0, "CHECKSUM"), ("isize", o + n - 4, 0, "CHECKSUM")):
            bad = imc.flip(whole, byte, bit)
            assert member_fails(bad, o, n)
            out.append(case("damage/member%d/%s" % (k, part), whole, ranges, read_file=bad, expect={i: (kind, k) for i in hit[k]}))
    # damage in members no range touches: every read succeeds
    quiet = [(outs[1] + 10, outs[3] + 20 - outs[1] - 10)]
    for k in (0, 4):
        bad = imc.flip(whole, st[k] + 18 + 7, 2)
        assert member_fails(bad, st[k], len(parts[k]))
        out.append(case("damage/untouched%d" % k, whole, quiet, read_file=bad))
    # a BSIZE that lies, read through the table of the true file: the decode never looks at it
    bad = imc.flip(whole, st[2] + 16, 0)
    out.append(case("damage/bsize_stale_index", whole, ranges, read_file=bad, index="members"))
    # an ISIZE that lies, in the index built from the lying file: the touched liar is TABLE, a range in front of it succeeds, and a
    # range behind it is shifted without notice (the header says so)
    for name, lie in (("small", -7), ("large", 7)):
        liar = b"".join(parts[:2] + (imc.bgzf(d[2], isize=len(d[2]) + lie),) + parts[3:])
        o2 = outs[2]
        rs = [(outs[1] + 10, len(d[1]) + 50), (5, 100), (outs[1], len(d[1])), (outs[3] + lie + 1, 40), (o2, 1), (o2 + len(d[2]) + lie - 1, 1)]
        out.append(case("damage/isize_too_%s" % name, liar, rs, expect={0: ("TABLE", 2), 4: ("TABLE", 2), 5: ("TABLE", 2)}))
    return out


def refusals():
    """files the index build refuses: (name, file, report.out_pos)"""
    d, parts = damage_parts()
    whole = b"".join(parts)
    st = imc.starts(parts)
    plain = imc.gz(imc.text(0, 300))
    return [
        ("refuse/plain_member_in_the_middle", b"".join(parts[:2]) + plain + b"".join(parts[2:]), len(d[0]) + len(d[1])),
        ("refuse/plain_member_first", plain + whole, 0),
        ("refuse/trailing_garbage", whole + b"\x1f\x8b\x08\x04garbage", sum(map(len, d))),
        ("refuse/one_trailing_byte", whole + b"\0", sum(map(len, d))),
        ("refuse/empty_file", b"", 0),
        ("refuse/truncated_in_the_last_member", whole[:st[4] + 40], sum(map(len, d[:4]))),
        ("refuse/truncated_in_a_header", whole[:st[3] + 9], sum(map(len, d[:3]))),
        # (a walker hops over the liar and reads its ISIZE where the lie says the trailer is)
        ("refuse/bsize_lies", imc.flip(whole, st[2] + 16, 0), claimed_prefix(imc.flip(whole, st[2] + 16, 0))),
        ("refuse/bsize_lies_large", b"".join(parts[:2] + (imc.bgzf(d[2], bsize_delta=100),) + parts[3:]),
         claimed_prefix(b"".join(parts[:2] + (imc.bgzf(d[2], bsize_delta=100),) + parts[3:]))),
    ]


@functools.lru_cache(maxsize=None)
def corpus():
    out = residues() + boundaries() + alignments() + spans() + shared() + budgets() + damage()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in corpus() if c.name == name)


# ---- what the case list claims -------------------------------------------------------------------------------------------------
def position_class(p, z, u):
    """where byte u lies inside the member [p, p + z): 'only' (z == 1), 'first', 'last' or 'inside'"""
    return "only" if z == 1 else "first" if u == p else "last" if u == p + z - 1 else "inside"


def coverage(cases=None):
    """(the (class of the first byte in its member, class of the last byte in its member) pairs of all successful ranges, the
    (dst % 16, src % 16) pairs of all pieces with the set of their lengths, the numbers of members single ranges touch)"""
    ends, pairs, lens, spans_ = set(), set(), set(), set()
    for c in cases or corpus():
        if c.read_file != c.file or c.index != "build":
            continue
        tab = table(c)
        for i, (off, length) in enumerate(c.ranges):
            ks = touched(tab, off, length)
            spans_.add(len(ks))
            if not ks:
                continue
            got = min(length, tab[-1][2] + tab[-1][3] - off)
            ends.add((position_class(tab[ks[0]][2], tab[ks[0]][3], off), position_class(tab[ks[-1]][2], tab[ks[-1]][3], off + got - 1)))
            if c.aligns is not None:
                for k in ks:
                    lo, hi = max(off, tab[k][2]), min(off + got, tab[k][2] + tab[k][3])
                    pairs.add(((c.aligns[i] + lo - off) % 16, (lo - tab[k][2]) % 16))
                    lens.add(hi - lo)
    return ends, pairs, lens, spans_
