"""The seek points on the host (deflate-rs_amd/csrc/inflate_seek.h through tests/inflseek): every case of inflate_seek_cases.py builds
at every spacing to the point list the rule gives, and every range read from it is zlib's slice of the stream -- the bytes, the
count, the untouched rest of the buffer and the canary --, alone and in batches, in one piece and in pieces; damage after the build
is noticed where a read decodes it and nowhere else; a wrong table, a wrong trailer and a truncated stream give no index; the two
mutants of the decisions are caught; and the stand-alone sanitizer program runs clean over the corpus.  No GPU."""
import os

import pytest

import inflate_seek_cases as sc
import inflseek_binding as sb

FILL = bytes([sb.FILL])


def build(c, spacing, group=sb.GROUP_DEFAULT, mutant=0):
    ix = sb.Index(c.stream, c.wrapper, c.table, spacing, group, mutant)
    assert ix.rc == sb.OK, (c.name, spacing, ix.report)
    return ix


def check(c, ranges, res, what):
    """every result of a clean stream against zlib's slice"""
    n = len(c.want)
    for (off, ln), (rc, got, rep, buf, canary) in zip(ranges, res):
        want = c.want[off:off + ln]
        assert rc == sb.OK and got == len(want) == min(ln, max(n - off, 0)), (c.name, what, off, ln, rc, got, rep)
        assert buf[:got] == want and buf[got:] == FILL * (ln - got) and canary, (c.name, what, off, ln)
        assert (rep["status"], rep["out_len"], rep["out_pos"]) == ("OK", got, min(off, n) + got), (c.name, what, off, ln, rep)


@pytest.mark.parametrize("spacing", sc.SPACINGS)
@pytest.mark.parametrize("name", [c.name for c in sc.corpus()])
def test_every_case_builds_its_points_and_reads_zlibs_bytes(name, spacing):
    c = sc.by_name(name)
    ix = build(c, spacing)
    pts = sc.points(c.table, spacing)
    assert ix.points() == pts and pts[0] == (0, 0), (name, spacing)
    if len(c.table) == 1 or spacing > len(c.want):
        assert len(pts) == 1
    assert ix.info() == dict(total=len(c.want), n_entries=len(c.table), n_points=len(pts), spacing=spacing, device_bytes=32768 * (len(pts) - 1),
                             stream_len=len(c.stream), wrapper=c.wrapper)
    assert (ix.report["status"], ix.report["out_len"]) == ("OK", len(c.want))
    ranges = sc.ranges(c, spacing)
    rc, res, counts, stray = ix.read_batch(ranges)
    assert rc == sb.OK and stray == 0 and counts["sets"] == 1
    check(c, ranges, res, "batch")
    for k, (off, ln) in enumerate(ranges):  # one by one: the same
        if c.full or k % 5 == 0:
            one = ix.read(off, ln)
            assert one[:5] == res[k], (name, spacing, off, ln)
            if ln == 1 and off < len(c.want):  # a byte costs the entries from its point to its own, not the stream's
                assert one[5] == dict(entries=sc.decoded(c.table, spacing, off), symbols=off + 1 - max(p for _b, p in pts if p <= off),
                                      steps=sc.decoded(c.table, spacing, off), sets=1), (name, spacing, off, one[5])
    assert sb.lib().inflseek_unfenced_loads() == 0


def test_a_byte_near_the_end_costs_the_entries_behind_its_point():
    c = sc.by_name("cut:lengths/w0")
    assert len(c.want) > 300000 and len(c.table) == 24
    ix = build(c, sc.WIN)
    last = sc.points(c.table, sc.WIN)[-1][1]
    for off, entries in ((len(c.want) - 70, 1), (len(c.want) - 1, 3)):  # (behind the last point: 10 000 bytes, none, 63)
        counts = ix.read(off, 1)[5]
        assert counts == dict(entries=entries, symbols=off + 1 - last, steps=entries, sets=1) and sc.decoded(c.table, sc.WIN, off) == entries


@pytest.mark.parametrize("name", ["cut:lengths/w0", "cut:first_token_32768_and_1/w0", "text:l6/w0"])
def test_every_offset_class_meets_every_pointer_class(name):
    c = sc.by_name(name)
    ix = build(c, sc.WIN)
    al = sc.alignments(c, sc.WIN)
    assert {(off % 16, a) for off, _ln, a in al} == {(i, a) for i in range(16) for a in range(8)}
    ranges = [(off, ln) for off, ln, _a in al]
    rc, res, _counts, stray = ix.read_batch(ranges, aligns=[a for _o, _l, a in al])
    assert rc == sb.OK and stray == 0
    check(c, ranges, res, "alignments")


@pytest.mark.parametrize("name", ["cut:lengths/w0", "text:l6/w2", "seek:oracle:pg11x3/default/w0"])
def test_a_range_longer_than_the_budget_goes_in_pieces(name):
    c = sc.by_name(name)
    ix = build(c, sc.WIN, group=sb.GROUP_MIN)
    assert ix.points() == sc.points(c.table, sc.WIN)  # (the groups of the build do not move the points)
    ranges = [sc.LONG, (0, len(c.want)), (len(c.want) // 2, 70000)]
    rc, res, counts, stray = ix.read_batch(ranges, group=sb.GROUP_MIN)
    assert rc == sb.OK and stray == 0 and counts["sets"] >= 4
    check(c, ranges, res, "pieces")
    assert ix.read(*sc.LONG, group=sb.GROUP_MIN)[5]["sets"] >= 2


@pytest.mark.parametrize("name", ["cut:lengths/w1", "cut:copies_of_copies/w0", "text:l9/w0"])
def test_batches_equal_single_reads(name):
    c = sc.by_name(name)
    ix = build(c, sc.WIN)
    for ranges in sc.batches(c, sc.WIN):
        rc, res, counts, stray = ix.read_batch(ranges)
        assert rc == sb.OK and stray == 0 and counts["sets"] == 1
        check(c, ranges, res, "batch of %d" % len(ranges))
        assert [ix.read(off, ln)[:5] for off, ln in ranges] == res


def test_damage_after_the_build_is_noticed_where_it_is_decoded():
    c = sc.by_name("cut:lengths/w0")
    ix = build(c, sc.WIN)
    (off, ln), flips = sc.damage(c, sc.WIN)
    failed = {"lead": 0, "inside": 0, "behind": 0, "outside": 0}
    for kind, bit in flips:
        rc, got, rep, buf, canary, _counts, stray = ix.read(off, ln, stream=sc.flipped(c.stream, bit))
        assert canary and stray == 0
        if kind == "outside":
            assert (rc, got, buf) == (sb.OK, ln, c.want[off:off + ln]), (kind, bit, rep)
            continue
        if rc == sb.E_DATA:
            failed[kind] += 1
            assert rep["status"] != "OK" and got == min(max(rep["out_pos"], off) - off, ln) and rep["out_len"] == 0, (kind, bit, rep)
            if kind == "lead":
                assert rep["out_pos"] < off and got == 0
            if kind == "behind":
                assert got == ln and buf == c.want[off:off + ln]  # the failure lies behind the range: its bytes are whole
        else:
            assert got == ln
        assert buf[got:] == FILL * (ln - got), (kind, bit)
        # a neighbour in the same batch, decoded from another point, is not disturbed
        rc2, res, _c, _s = ix.read_batch([(off, ln), (0, 100)], stream=sc.flipped(c.stream, bit))
        assert res[0][:4] == (rc, got, rep, buf) and res[1][0] == sb.OK and res[1][3] == c.want[:100] and rc2 == rc
    assert min(failed["lead"], failed["inside"], failed["behind"]) >= 1 and failed["outside"] == 0, failed


def test_a_failing_piece_stops_its_range():
    """a range in pieces, damage in its second piece: nothing is stored at or beyond the failure, the pieces behind it included"""
    c = sc.by_name("cut:lengths/w0")
    ix = build(c, sc.WIN)
    pos = [p for _b, p in sc.points(c.table, sc.WIN)]
    k = sc.entry_of(c.table, pos[3] + 10)
    hit = 0
    for f in (0.3, 0.5, 0.7):
        bit = c.table[k][0] + int((c.table[k + 1][0] - c.table[k][0]) * f)
        rc, got, rep, buf, canary, counts, stray = ix.read(1000, 250000, stream=sc.flipped(c.stream, bit), group=sb.GROUP_MIN)
        assert canary and stray == 0 and counts["sets"] >= 3
        if rc == sb.E_DATA:
            hit += 1
            assert pos[3] <= rep["out_pos"] < pos[4] and got == rep["out_pos"] - 1000
            assert buf[:pos[3] - 1000] == c.want[1000:pos[3]] and buf[got:] == FILL * (250000 - got)
    assert hit >= 1


def test_streams_that_give_no_index():
    c = sc.by_name("cut:lengths/w0")
    t = [list(x) for x in c.table]
    t[5][1] += 1
    t[6][1] -= 1
    ix = sb.Index(c.stream, 0, [tuple(x) for x in t], sc.WIN)
    assert (ix.rc, ix.report["status"]) == (sb.E_DATA, "TABLE")
    for name, at in (("cut:lengths/w1", -2), ("cut:lengths/w2", -6), ("cut:lengths/w2", -1)):  # Adler-32, CRC-32, ISIZE
        c = sc.by_name(name)
        m = bytearray(c.stream)
        m[at] ^= 0x10
        for group in (sb.GROUP_DEFAULT, sb.GROUP_MIN):  # (sums folded over one group and over several)
            ix = sb.Index(bytes(m), c.wrapper, c.table, sc.WIN, group)
            assert (ix.rc, ix.report["status"], ix.report["out_pos"]) == (sb.E_DATA, "CHECKSUM", len(c.want)), (name, at, ix.report)
            assert sb.Index(c.stream, c.wrapper, c.table, sc.WIN, group).rc == sb.OK
    c = sc.by_name("cut:lengths/w0")
    ix = sb.Index(c.stream[:len(c.stream) // 2], 0, c.table, sc.WIN)
    assert ix.rc == sb.E_DATA and ix.report["status"] in ("TRUNCATED", "TABLE", "STORED", "CODE")
    for spacing in (1, sc.WIN - 1, (1 << 30) + 1, 1 << 31):
        assert sb.Index(c.stream, 0, c.table, spacing).rc == sb.E_ARG
    assert sb.Index(c.stream, 0, c.table, 0).info()["spacing"] == 1 << 20  # the default


def test_the_mutants_are_caught():
    # the point rule off by one entry: a point list that is not the rule's
    wrong = 0
    for name in ("cut:lengths/w0", "text:l6/w0", "cut:first_token_32768_and_1/w0"):
        c = sc.by_name(name)
        wrong += build(c, sc.WIN, mutant=sb.MUTANT_POINTS).points() != sc.points(c.table, sc.WIN)
    assert wrong >= 2
    # a resolve without the lower bound: stores in front of the range's buffer
    c = sc.by_name("cut:lengths/w0")
    ix = build(c, sc.WIN, mutant=sb.MUTANT_RESOLVE)
    p = sc.points(c.table, sc.WIN)[2][1]
    assert ix.read(p + 1000, 500)[6] >= 1000
    assert build(c, sc.WIN).read(p + 1000, 500)[6] == 0


def test_the_standalone_sanitizer_program_runs_clean(tmp_path):
    cases = []
    for c in sc.corpus():
        for spacing in (sc.WIN, 100000):
            if spacing != sc.WIN and not c.full:
                continue
            ranges = sc.ranges(c, spacing)[::1 if c.full else 3] + [(off, ln) for off, ln, _a in sc.alignments(c, spacing)[::9]]
            cases.append((c.stream, c.wrapper, c.table, spacing, sb.GROUP_DEFAULT, c.want, ranges, None))
    c = sc.by_name("cut:lengths/w0")
    cases.append((c.stream, 0, c.table, sc.WIN, sb.GROUP_MIN, c.want, [sc.LONG, (0, len(c.want))], None))
    (off, ln), flips = sc.damage(c, sc.WIN)
    for _kind, bit in flips:
        cases.append((c.stream, 0, c.table, sc.WIN, sb.GROUP_MIN, c.want, [(off, ln), (1000, 250000)], sc.flipped(c.stream, bit)))
    cases.append((c.stream[:-100] + bytes(100), 0, c.table, sc.WIN, sb.GROUP_DEFAULT, c.want, [(0, 10)], None))  # (no index)
    path = os.path.join(str(tmp_path), "corpus.bin")
    sb.write_corpus(path, cases)
    status, out = sb.run_fuzz(path)
    assert status == 0, out
    assert "%d cases" % len(cases) in out and " 1 refused" in out
