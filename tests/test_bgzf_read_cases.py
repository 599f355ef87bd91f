"""CPU-only: the host build of the BGZF reads (tests/bgzfread, bgzf_read.h) against zlib's slices on every case of
bgzf_read_cases.py -- return value, got, report, bytes, the untouched fill around and inside `out`, the plan's counts --, the three
mutants each caught by a named case, what the case list claims to cover, the index build's refusals, from_members' rules, virtual
offsets, and the stand-alone sanitizer program over the corpus."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import bgzf_read_cases as brc  # noqa: E402
import bgzfread_binding as hb  # noqa: E402

CASES = brc.corpus()
STRUCTURAL = ("FRAME", "BTYPE", "STORED", "LENGTHS", "CODE", "DISTANCE", "TRUNCATED", "TRAILER")


def index_of(c):
    if c.index == "members":
        ix = hb.Index(members=[t + (0, 0) for t in brc.table(c)], file_len=len(c.file))
        ix.file = c.file
    else:
        ix = hb.Index(file=c.file)
    assert ix.rc == hb.OK
    return ix


def check_range(c, tab, img, i, res):
    """one range's result against the judge"""
    off, length = c.ranges[i]
    st, got, rep, buf, guards = res
    total = tab[-1][2] + tab[-1][3]
    full = 0 if off >= total else min(length, total - off)
    assert guards, (c.name, i)
    if i not in c.expect:
        assert st == hb.OK and got == full, (c.name, i, st, got, rep)
        assert rep["status"] == "OK" and rep["out_len"] == got and rep["out_pos"] == off + got and rep["bit"] == 0
        ks = brc.touched(tab, off, length)
        assert rep["n_blocks"] >= len(ks) and rep["n_blocks"] == rep["n_stored"] + rep["n_fixed"] + rep["n_dynamic"]
        assert (rep["n_blocks"] == 0) == (not ks)
        assert buf[:got] == img[off:off + got], (c.name, i)
        assert buf[got:] == bytes([hb.FILL]) * (len(buf) - got), (c.name, i)
        return
    kind, k = c.expect[i]
    _o, _n, p, z = tab[k]
    assert st == hb.E_DATA, (c.name, i, st, rep)
    if kind == "ANY":
        assert rep["status"] in STRUCTURAL + ("CHECKSUM", "TABLE") and p <= rep["out_pos"] <= p + z, (c.name, i, rep)
    else:
        assert rep["status"] == kind and rep["out_pos"] == p, (c.name, i, rep)
    assert rep["out_len"] == 0 and rep["n_blocks"] == 0
    assert got == min(max(rep["out_pos"], off) - off, length)
    if rep["out_pos"] == p:  # the members in front of the failing one are the file's
        assert buf[:got] == img[off:off + got], (c.name, i)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_against_zlib(c):
    ix = index_of(c)
    tab, img = brc.table(c), brc.image(c)
    assert [(m["in_off"], m["in_len"], m["out_off"], m["out_len"]) for m in ix.members()] == tab
    assert ix.info() == dict(total=len(img), n_members=len(tab), file_len=len(c.file), max_out_len=max(t[3] for t in tab))
    rc, res, counts = ix.read_batch(c.ranges, file=c.read_file, budget=c.budget, aligns=c.aligns)
    assert counts == brc.plan_counts(tab, c.ranges, c.budget), c.name
    firsts = [r[0] for r in res if r[0] != hb.OK]
    assert rc == (firsts[0] if firsts else hb.OK)
    for i in range(len(c.ranges)):
        check_range(c, tab, img, i, res[i])
    # each range alone: the same status, got, report and bytes (a failing range disturbs no neighbour, and no neighbour helps one)
    step = 1 if len(c.ranges) <= 64 else 7
    for i in range(0, len(c.ranges), step):
        one = ix.read(c.ranges[i][0], c.ranges[i][1], file=c.read_file, budget=c.budget, align=0 if c.aligns is None else c.aligns[i])
        assert one[:3] == res[i][:3] and one[3][:one[1]] == res[i][3][:one[1]] and one[4], (c.name, i)  # (out[got, len) is unspecified)
        assert one[5] == brc.plan_counts(tab, [c.ranges[i]], c.budget)
    assert hb.lib().bgzfread_unfenced_loads() == 0


def test_what_the_case_list_claims():
    ends, pairs, lens, spans = brc.coverage()
    classes = ("first", "inside", "last")
    assert {(a, b) for a in classes for b in classes} <= ends  # every (start inside member, end inside member) class
    assert {("only", "only"), ("only", "first"), ("last", "only")} <= ends
    assert pairs == {(d, s) for d in range(16) for s in range(16)}
    assert set(range(1, 49)) <= lens
    assert {0, 1, 2, 3} <= spans and max(spans) == sum(1 for n in brc.SMALL_LENS if n)
    tab = brc.claims(brc.small_file())
    assert [t[3] for t in tab] == list(brc.SMALL_LENS)
    assert any(a[3] == 0 and b[3] == 0 for a, b in zip(tab, tab[1:])) and tab[0][3] == 0 and tab[-1][3] == 0
    assert max(t[3] for t in brc.claims(brc.big_file())) == 65280
    names = {c.name for c in CASES}
    for k in range(5):
        for part in ("magic", "cm", "data", "data0", "crc", "isize"):
            assert "damage/member%d/%s" % (k, part) in names
    assert hb.lib().bgzfread_piece_size() == 24 and hb.lib().bgzfread_set_members() == brc.SET_MEMBERS


def test_plan_counts_of_the_named_cases():
    def counts(name):
        c = brc.by_name(name)
        return index_of(c).read_batch(c.ranges, budget=c.budget)[2]

    # one range covers the member, another only cuts it: the member goes to scratch, once, with two pieces
    assert counts("shared/covered_and_cut") == dict(distinct=1, in_place=0, scratch=1, pieces=2, sets=1)
    assert counts("shared/cut_and_covered") == dict(distinct=3, in_place=0, scratch=3, pieces=4, sets=1)
    assert counts("shared/three_in_one") == dict(distinct=1, in_place=0, scratch=1, pieces=3, sets=1)
    assert counts("shared/whole_twice") == dict(distinct=1, in_place=0, scratch=1, pieces=2, sets=1)
    # slots of 304, 65280 and 704 bytes under 65536: neither neighbour fits beside the large member
    assert counts("budget/three_sets") == dict(distinct=3, in_place=0, scratch=3, pieces=3, sets=3)
    assert counts("budget/big_alone") == dict(distinct=1, in_place=0, scratch=1, pieces=1, sets=1)
    assert counts("budget/big_in_place") == dict(distinct=3, in_place=1, scratch=2, pieces=2, sets=1)
    c = brc.by_name("spans/small")
    n = sum(1 for z in brc.SMALL_LENS if z)
    assert index_of(c).read(0, sum(brc.SMALL_LENS))[5] == dict(distinct=n, in_place=n, scratch=0, pieces=0, sets=1)


def results(c, mutant):
    return index_of(c).read_batch(c.ranges, file=c.read_file, budget=c.budget, aligns=c.aligns, mutant=mutant)


def test_mutant_in_place_ignores_sharing_is_caught():
    c = brc.by_name("shared/covered_and_cut")
    img = brc.image(c)
    _rc, good, counts = results(c, 0)
    _rc, bad, bad_counts = results(c, hb.MUTANT_SHARING)
    assert all(r[3][:r[1]] == img[off:off + r[1]] for r, (off, _n) in zip(good, c.ranges))
    assert bad_counts["in_place"] == 1 and counts["in_place"] == 0
    assert any(r[3][:r[1]] != img[off:off + r[1]] for r, (off, _n) in zip(bad, c.ranges))


def test_mutant_piece_copy_off_by_one_at_the_seam_is_caught():
    c = brc.by_name("alignments")
    img = brc.image(c)
    _rc, bad, _counts = results(c, hb.MUTANT_SEAM)
    wrong = [i for i, (r, (off, _n)) in enumerate(zip(bad, c.ranges)) if r[3][:r[1]] != img[off:off + r[1]]]
    assert wrong
    # exactly the pieces with bytes in front of a 16-byte boundary of the destination and a whole granule behind it
    for i, (_off, n) in enumerate(c.ranges):
        head = -c.aligns[i] % 16
        assert (i in wrong) == (head > 0 and n - head >= 16), (i, n, c.aligns[i])


def test_mutant_accept_without_the_length_test_is_caught():
    c = brc.by_name("damage/isize_too_large")
    _rc, good, _counts = results(c, 0)
    _rc, bad, _counts = results(c, hb.MUTANT_LENGTH)
    assert good[0][2]["status"] == "TABLE" and bad[0][2]["status"] == "CHECKSUM"
    c = brc.by_name("damage/isize_too_small")
    assert results(c, 0)[1][0][2]["status"] == "TABLE" and results(c, hb.MUTANT_LENGTH)[1][0][0] == hb.OK


@pytest.mark.parametrize("name,file,pos", brc.refusals(), ids=[r[0] for r in brc.refusals()])
def test_index_build_refusals(name, file, pos):
    for span in (hb.SPAN_DEFAULT, 64):
        ix = hb.Index(file=file, span=span)
        assert ix.rc == hb.E_DATA
        assert ix.report == dict(status="FRAME", bit=0, out_pos=pos, out_len=0, n_blocks=0, n_stored=0, n_fixed=0, n_dynamic=0)


def test_index_build_at_small_spans():
    want = brc.claims(brc.small_file())
    for span in (16, 64, 100, 4096):
        ix = hb.Index(file=brc.small_file(), span=span)
        assert ix.rc == hb.OK and [(m["in_off"], m["in_len"], m["out_off"], m["out_len"]) for m in ix.members()] == want
        assert all(m["flags"] == 1 and m["status"] == "OK" for m in ix.members())
        assert ix.report["out_len"] == ix.report["out_pos"] == sum(brc.SMALL_LENS) and ix.report["n_blocks"] == 0


def from_members_cases():
    """(name, rows, file_len, accepted?)"""
    good = [(0, 30, 0, 5), (30, 18, 5, 0), (48, 100, 5, 70000)]
    def edit(k, **kw):
        rows = [dict(zip(("in_off", "in_len", "out_off", "out_len"), r)) for r in good]
        rows[k].update(kw)
        return rows
    return [
        ("good", good, 148, True),
        ("good_flags_not_required", edit(1, flags=0), 148, True),
        ("no_members", [], 0, False),
        ("a_status", edit(1, status=12), 148, False),
        ("first_in_off", edit(0, in_off=1, in_len=29), 148, False),
        ("in_gap", edit(1, in_off=31, in_len=17), 148, False),
        ("in_overlap", edit(1, in_off=29), 148, False),
        ("last_ends_short", good, 149, False),
        ("last_ends_beyond", good, 147, False),
        ("first_out_off", edit(0, out_off=1, out_len=4), 148, False),
        ("out_gap", edit(2, out_off=6), 148, False),
        ("out_overlap", edit(2, out_off=4), 148, False),
        ("in_len_17", [(0, 17, 0, 0), (17, 131, 0, 9)], 148, False),
        ("in_len_18", [(0, 18, 0, 0), (18, 130, 0, 9)], 148, True),
    ]


FROM_MEMBERS = from_members_cases()


@pytest.mark.parametrize("name,rows,file_len,ok", FROM_MEMBERS, ids=[r[0] for r in FROM_MEMBERS])
def test_from_members_rules(name, rows, file_len, ok):
    ix = hb.Index(members=rows, file_len=file_len)
    assert ix.rc == (hb.OK if ok else hb.E_ARG)
    if ok:
        assert ix.info()["n_members"] == len(rows) and ix.info()["file_len"] == file_len


def test_virtual_offsets():
    ix = hb.Index(file=brc.small_file())
    tab = brc.claims(brc.small_file())
    total, file_len = tab[-1][2] + tab[-1][3], len(brc.small_file())
    for k, (o, _n, p, z) in enumerate(tab):
        if z:  # every member start, its last byte, and back
            for u in (p, p + z - 1, p + z // 2):
                assert ix.voffset(u) == (hb.OK, o << 16 | (u - p))
                assert ix.uoffset(o << 16 | (u - p)) == (hb.OK, u)
            assert ix.uoffset(o << 16 | z)[0] == hb.E_ARG  # the low bits at the member's out_len
        else:  # an empty member: never chosen, and only its offset 0 is taken
            assert ix.uoffset(o << 16) == (hb.OK, p)
            assert ix.uoffset(o << 16 | 1)[0] == hb.E_ARG
            assert ix.voffset(p)[1] >> 16 != o
    assert ix.voffset(total) == (hb.OK, file_len << 16) and ix.uoffset(file_len << 16) == (hb.OK, total)
    assert ix.voffset(total + 1)[0] == hb.E_ARG and ix.uoffset(file_len << 16 | 1)[0] == hb.E_ARG
    assert ix.uoffset((tab[5][0] + 1) << 16)[0] == hb.E_ARG and ix.uoffset((file_len + 1) << 16)[0] == hb.E_ARG  # no member start
    # a member larger than 64 KiB, or one at or beyond 2^48, has no virtual offset
    big = hb.Index(members=[(0, 100, 0, 65536), (100, 100, 65536, 65537), (200, 100, 131073, 1)], file_len=300)
    assert big.voffset(65535) == (hb.OK, 65535) and big.voffset(65536)[0] == hb.E_UNSUPPORTED and big.voffset(131073) == (hb.OK, 200 << 16)
    far = hb.Index(members=[(0, 1 << 48, 0, 10), (1 << 48, 100, 10, 10)], file_len=(1 << 48) + 100)
    assert far.voffset(9)[0] == hb.OK and far.voffset(10)[0] == hb.E_UNSUPPORTED and far.voffset(20)[0] == hb.E_UNSUPPORTED


def test_a_claim_above_the_budget_is_unsupported():
    f = brc.big_file()
    d = brc.true_members(f)
    tab = brc.claims(f)
    big = hb.Index(members=[tab[0], (tab[1][0], tab[1][1], tab[1][2], 65552)] + [(o, n, p + 272, z) for o, n, p, z in tab[2:]], file_len=len(f))
    big.file = f
    rc, res, counts = big.read_batch([(5, 10), (400, 10), (300, 65552)], budget=hb.GROUP_MIN)
    assert rc == hb.E_UNSUPPORTED and [r[0] for r in res] == [hb.OK, hb.E_UNSUPPORTED, hb.E_UNSUPPORTED]
    assert res[0][3] == d[0][5:15] and res[1][1] == 0 and counts["distinct"] == 1
    # in place the claim needs no scratch: the member is decoded, and found shorter than claimed
    rc, res, _counts = big.read_batch([(300, 65552)], budget=hb.GROUP_MIN)
    assert rc == hb.E_DATA and res[0][2]["status"] == "TABLE" and res[0][2]["out_pos"] == 300 and res[0][1] == 0 and res[0][4]


def test_sanitizer_program_runs_the_corpus(tmp_path):
    path = str(tmp_path / "corpus.bin")
    cases = []
    for c in CASES:
        if c.index != "build":
            continue
        damaged = c.read_file if c.read_file != c.file else None
        if damaged is None and c.expect:
            continue  # (a lying file: its reads are not zlib's; the host build ran it above)
        cases.append((c.file, damaged, c.budget, brc.image(c), [r for r in c.ranges if r[1] <= hb.ROOM_MAX]))
    for _name, file, _pos in brc.refusals():
        cases.append((file, None, hb.GROUP_MIN, b"", [(0, 10)]))
    hb.write_corpus(path, cases)
    status, out = hb.run_fuzz(path)
    assert status == 0, out
    assert "%d cases" % len(cases) in out and "%d refused" % len(brc.refusals()) in out
