"""The cases of tests/checksum_cases.py on the CPU.  The references in Python integers agree with zlib; the unmutated models of the
checksum kernels give the reference on every case -- sizes x patterns x offsets, none left out; every mutant of the models (one
rule of the kernels wrong) is noticed by at least one case of the lists that tests/test_checksum_gpu.py runs; and
mi355_checksum_combine, the host arithmetic that joins flush segments and ranks, equals both combine references and zlib.  With
that, a failure of the GPU test on a case points at what only the GPU runs.  CPU only."""
import os
import random
import sys
import zlib

import pytest

import checksum_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

KINDS = ("adler", "crc")


def test_constants_and_lists():
    assert cc.kernel_constants() == {"ADLER_CHUNK": 16384, "CRC_CHUNK": 512, "CRC_PIECE": 128}
    for n in (16, 4096, cc.ADLER_CHUNK, 2 * cc.ADLER_CHUNK):
        assert {n - 1, n, n + 1} <= set(cc.ADLER_SIZES), n
    # `after` of a chunk next to 65521 and to 2 * 65521
    assert {n - cc.ADLER_CHUNK for n in cc.ADLER_SIZES} >= set(range(cc.BASE - 2, cc.BASE + 3)) | set(range(2 * cc.BASE, 2 * cc.BASE + 3))
    assert {n - 2 * cc.ADLER_CHUNK for n in cc.ADLER_SIZES} >= set(range(cc.BASE, cc.BASE + 3))
    for n in (16, cc.CRC_PIECE, 2 * cc.CRC_PIECE, 3 * cc.CRC_PIECE, cc.CRC_CHUNK, 2 * cc.CRC_CHUNK, 64 * cc.CRC_CHUNK, cc.CRC_TILE, 2 * cc.CRC_TILE):
        assert {n - 1, n, n + 1} <= set(cc.CRC_SIZES), n
    assert max(cc.ADLER_SIZES + cc.CRC_SIZES) <= cc.MAX_PATTERN
    assert cc.onehot_positions(1) == [0] and cc.onehot_positions(0) == []
    assert cc.onehot_positions(16385) == [0, 12288, 15872, 16256, 16368, 16383, 16384]
    assert cc.onehot_positions(4097)[-3:] == [4080, 4095, 4096]
    assert cc.hot_chunks(131073) == [0, 63, 64, 255, 256] and cc.hot_chunks(513) == [0, 1] and cc.hot_chunks(0) == []


def test_placement_guards_and_offsets():
    buf, cases = cc.arena("adler", "ff")
    assert len(cases) == len(cc.ADLER_SIZES) * len(cc.OFFSETS)
    end = 0
    for c in cases:
        assert c.at % 32 == c.off and c.at - end >= cc.GUARD, c
        assert (buf[end:c.at] == cc.GUARD_BYTE).all() and (buf[c.at:c.at + c.n] == 0xFF).all()
        end = c.at + c.n
    assert len(buf) - end >= cc.GUARD and (buf[end:] == cc.GUARD_BYTE).all()
    assert {c.at % 16 for c in cases} == {0, 1, 3, 4, 8, 15}


def test_combine_references_against_zlib():
    """before anything relies on them: both references on real concatenations"""
    rnd = random.Random(20)
    for k in range(120):
        la, lb = rnd.choice((0, 1, 2, 511, 65520, 65521, 70000, rnd.randrange(200000))), rnd.choice((0, 1, 3, 512, 65521, 131073, rnd.randrange(200000)))
        a = rnd.getrandbits(8 * la).to_bytes(la, "little") if k % 3 else bytes([0xFF]) * la
        b = rnd.getrandbits(8 * lb).to_bytes(lb, "little") if k % 5 else bytes([0xFF]) * lb
        assert cc.adler_combine_ref(zlib.adler32(a), zlib.adler32(b), lb) == zlib.adler32(a + b), (la, lb)
        assert cc.crc_combine_ref(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)


def test_closed_forms_against_zlib():
    for v in (0, 1, 0xEE, 0xFF):
        for n in (0, 1, 5551, 5552, 5553, 65521, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (3 << 20) + 77, (5 << 20)):
            data = bytes([v]) * n
            assert cc.adler_const(n, v) == zlib.adler32(data), (n, v)
            assert cc.crc_const(n, v) == zlib.crc32(data), (n, v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_model_equals_reference_on_every_case(kind, family):
    buf, cases = cc.arena(kind, family)
    assert {(c.n, c.off) for c in cases} == {(n, off) for n in cc.SIZES[kind] for off in cc.OFFSETS if n or family not in ("onehot", "hot")}
    stray = []
    got = cc.model_many(kind, buf, cases, stray=stray)
    for c, g in zip(cases, got):
        data = cc.case_bytes(buf, c)
        want = cc.reference(kind, data)
        assert g == want, "%s: model %08x, zlib %08x" % (cc.case_id(c), g, want)
        if family in ("zeros", "ff"):
            const = (cc.adler_const if kind == "adler" else cc.crc_const)(c.n, 0xFF if family == "ff" else 0)
            assert const == want, cc.case_id(c)
    assert not any(stray)  # the kernels' bounds tests keep every read inside the n bytes


MUTANT_OFFSETS = (0, 1)  # (one aligned and one unaligned placement: what the GPU test runs holds these)


@pytest.mark.parametrize("kind,mutant", [("adler", m) for m in cc.ADLER_MUTANTS] + [("crc", m) for m in cc.CRC_MUTANTS])
def test_mutant_of_the_model_is_noticed(kind, mutant):
    """A mutant is noticed by a case on which it gives another value than zlib.  crc_stage_unmasked cannot be: `here` bounds what the
    CRC loop takes from the staged bytes, so the bytes that a lane stages from behind n are never used, and the mask is there for the
    reads alone -- that mutant is noticed by the model's count of bytes read outside the n bytes, on every case that is no whole
    number of tiles."""
    what = dict(cc.ADLER_MUTANTS, **cc.CRC_MUTANTS)[mutant]
    table, by_value, by_reads = [], 0, 0
    for family in cc.FAMILIES:
        buf, cases = cc.arena(kind, family, MUTANT_OFFSETS)
        stray = []
        got = cc.model_many(kind, buf, cases, mutant, stray)
        wrong = [c for c, g in zip(cases, got) if g != cc.reference(kind, cc.case_bytes(buf, c))]
        strays = [c for c, s in zip(cases, stray) if s]
        by_value += len(wrong)
        by_reads += len(strays)
        table.append("  %-7s %4d of %4d by value, %4d by reads  %s" % (family, len(wrong), len(cases), len(strays),
                                                                        " ".join(cc.case_id(c) for c in (wrong or strays)[:3])))
    print("%s (%s):\n%s" % (mutant, what, "\n".join(table)))
    if mutant == "crc_stage_unmasked":
        assert by_value == 0 and by_reads, "no case notices: %s" % what
    else:
        assert by_value, "no case notices: %s" % what
        assert by_reads == 0 or mutant == "adler_tail_unmasked"


def test_thirteen_mutants():
    assert len(cc.ADLER_MUTANTS) == 7 and len(cc.CRC_MUTANTS) == 6


# ---- mi355_checksum_combine ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def combine():
    import deflate_amd
    if not os.path.exists(deflate_amd.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "deflate-rs_amd"), "-s"])
    L = deflate_amd.load()  # (no context: the library loads on a machine without a GPU)
    return lambda kind, a, b, n: L.mi355_checksum_combine(kind, a, b, n)


LENS = (0, 1, 65520, 65521, 65522, 2 * 65521, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7)


def test_combine_equals_the_references_on_the_edges(combine):
    rnd = random.Random(31)
    half = (0, 1, 65520, rnd.randrange(65521), rnd.randrange(65521))
    sums = [hi << 16 | lo for hi in half for lo in half]
    for s1 in sums:
        for s2 in sums:
            for n in LENS:
                assert combine(1, s1, s2, n) == cc.adler_combine_ref(s1, s2, n), (hex(s1), hex(s2), n)
    crcs = (0, 0xFFFFFFFF, rnd.getrandbits(32), rnd.getrandbits(32), 1, 0x80000000)
    for c1 in crcs:
        for c2 in crcs:
            for n in LENS:
                assert combine(2, c1, c2, n) == cc.crc_combine_ref(c1, c2, n), (hex(c1), hex(c2), n)
    for n in LENS:  # random sums at every length
        for _ in range(20):
            s1, s2 = (rnd.randrange(65521) << 16 | rnd.randrange(65521) for _ in range(2))
            assert combine(1, s1, s2, n) == cc.adler_combine_ref(s1, s2, n), (hex(s1), hex(s2), n)
            c1, c2 = rnd.getrandbits(32), rnd.getrandbits(32)
            assert combine(2, c1, c2, n) == cc.crc_combine_ref(c1, c2, n), (hex(c1), hex(c2), n)


def test_combine_on_real_splits_and_folds(combine):
    rnd = random.Random(32)
    bufs = []
    for family in cc.FAMILIES:
        n = rnd.choice((147428, 262145, 393217, 98291))
        bufs.append(cc.pattern(family, cc.details(family, n)[-1], n).tobytes())
    n_splits = 0
    for k in range(200):
        data = bufs[k % len(bufs)]
        cut = rnd.choice((0, 1, len(data) - 1, len(data), 65521, len(data) - 65521, rnd.randrange(len(data))))
        a, b = data[:cut], data[cut:]
        assert combine(1, zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(data), (k, cut)
        assert combine(2, zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), (k, cut)
        n_splits += 1
    assert n_splits == 200
    # k pieces folded left to right, from the checksum of nothing: the whole
    for data in bufs:
        for k in (1, 2, 3, 7, 16):
            cuts = sorted(rnd.randrange(len(data) + 1) for _ in range(k - 1))
            acc_a, acc_c = zlib.adler32(b""), zlib.crc32(b"")
            for lo, hi in zip([0] + cuts, cuts + [len(data)]):
                acc_a = combine(1, acc_a, zlib.adler32(data[lo:hi]), hi - lo)
                acc_c = combine(2, acc_c, zlib.crc32(data[lo:hi]), hi - lo)
            assert (acc_a, acc_c) == (zlib.adler32(data), zlib.crc32(data)), (k, cuts)


def test_batches_of_the_gpu_test_are_what_they_claim():
    specs = cc.batch_specs()
    sizes = [s[2] for s in specs]
    assert set(sizes) == set(cc.ADLER_SIZES) | set(cc.CRC_SIZES) and all(sizes.count(n) == 1 for n in set(sizes) if n)
    zeros = [k for k, n in enumerate(sizes) if n == 0]
    assert len(zeros) >= 3 and all(0 < k < len(sizes) - 1 and sizes[k - 1] and sizes[k + 1] for k in zeros)  # between full items
    assert {131071, 131072} <= set(sizes)  # 8 Adler workgroups, 1 CRC workgroup
    assert {s[0] for s in specs} == set(cc.BATCH_FAMILIES) and {s[3] for s in specs} == set(cc.OFFSETS)
    buf, cases = cc.build_arena(specs)
    for wrapper in (1, 2):
        for c in cases[::7]:
            data = cc.case_bytes(buf, c)
            s = cc.frame(data, wrapper, 0 if c.family == "random" else 6)
            assert zlib.decompressobj(15 if wrapper == 1 else 31).decompress(s) == data
            for which in (0, 1):
                with pytest.raises(zlib.error):
                    d = zlib.decompressobj(15 if wrapper == 1 else 31)
                    d.decompress(cc.flip_trailer(s, wrapper, which))
                    d.flush()
    enc = cc.encode_specs()
    assert {s[2] for s in enc} == {16383, 16384, 16385, 131071, 131072, 131073} and {s[3] for s in enc} == {0, 1}
    assert {s[0] for s in enc} == {"ff", "ramp", "onehot"}
