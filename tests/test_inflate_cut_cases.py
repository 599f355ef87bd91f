"""The cuts of a seek handle on the host (deflate-rs_amd/csrc/inflate_cut.h through tests/inflcut): for every case of
inflate_cut_cases.py and every cut_bytes the host build's cut list is the Python walk's, lane by lane and by the serial model; every
range read is zlib's slice and equals the read from a handle without cuts -- bytes, count, untouched rest, canary --, alone, in
batches and in pieces; the block counts of the cuts of a whole-stream read sum to the build's; damage after the build is rejected
where a cut decodes it; a mutated cut list never gives wrong bytes with OK; the three mutants die; the coverage table is complete;
and the stand-alone sanitizer program runs clean over the corpus.  No GPU."""
import os

import pytest

import inflate_cut_cases as cc
import inflcut_binding as cb

FILL = bytes([cb.FILL])
NAMES = [c.name for c in cc.corpus()]


def build(c, cut, group=cb.GROUP_DEFAULT, mutant=0, serial=False):
    ix = cb.Index(c.stream, c.wrapper, c.table, cc.SPACING, group, cut, mutant, serial)
    assert ix.rc == cb.OK, (c.name, cut, ix.report)
    return ix


def check(c, ranges, res, what):
    """every result of a clean stream against zlib's slice"""
    n = len(c.want)
    for (off, ln), (rc, got, rep, buf, canary) in zip(ranges, res):
        want = c.want[off:off + ln]
        assert rc == cb.OK and got == len(want) == min(ln, max(n - off, 0)), (c.name, what, off, ln, rc, got, rep)
        assert buf[:got] == want and buf[got:] == FILL * (ln - got) and canary, (c.name, what, off, ln)
        assert (rep["status"], rep["out_len"], rep["out_pos"]) == ("OK", got, min(off, n) + got), (c.name, what, off, ln, rep)


def test_the_coverage_table_is_complete():
    table = cc.coverage()
    cc.print_coverage(table)
    assert all(table[cell] for cell in cc.CELLS), [cell for cell in cc.CELLS if not table[cell]]
    # the streams that are ONE entry: every stored header behind the first is a cut; the fixed stream's cuts lie inside its blocks
    for cut in cc.CUT_BYTES:
        c = cc.by_name("stored/w0")
        places, _m, _end = cc.walk(c.raw, tuple(c.table))
        assert [x[0] for x in cc.cuts(c, cut)[0]] == [pl.bit for pl in places if pl.kind == "H0"] and len(c.table) == 1
        c = cc.by_name("fixed/w0")
        cl, on = cc.cuts(c, cut)
        assert len(c.table) == 1 and len({pl.hdr for pl in on}) >= 3 and all(pl.kind in "LME" for pl in on[1:]) and len(cl) > len(c.want) // cut // 2


@pytest.mark.parametrize("cut", cc.CUT_BYTES)
@pytest.mark.parametrize("name", NAMES)
def test_every_case_builds_the_walks_cuts_and_reads_zlibs_bytes(name, cut):
    c = cc.by_name(name)
    want, _on = cc.cuts(c, cut)
    # every cut boundary through the serial model; the thinned list through the form that replays every lane
    for serial in (True, False):
        ranges = cc.ranges(c, cut, every=serial)
        off0 = build(c, 0, serial=serial)
        rc0, res0, counts0, cuts0 = off0.read_batch(ranges)
        check(c, ranges, res0, "no cuts")
        assert off0.cuts() == [] and cuts0 == dict(cuts=0, symbols=counts0["symbols"], steps=0, launches=3 * counts0["sets"])
        ix = build(c, cut, serial=serial)
        assert ix.cuts() == want, (name, cut, serial)
        assert ix.report == off0.report  # the build's report does not depend on the key
        info = ix.info()
        assert (info["n_cuts"], info["surplus"], info["n_points"]) == (len(want), 0, off0.info()["n_points"])
        rc, res, counts, cuts = ix.read_batch(ranges)
        assert rc == cb.OK and counts == counts0 and cuts["launches"] == 4 * counts["sets"] and cuts["steps"] == cuts["cuts"] - counts["entries"]
        check(c, ranges, res, "batch")
        for r, r0 in zip(res, res0):  # ... and what the handle without cuts gives, the block counts aside
            assert r[:2] == r0[:2] and r[3:] == r0[3:]
        for k, (off, ln) in enumerate(ranges):
            if k % (97 if serial else 7) == 0:
                assert ix.read(off, ln)[:5] == res[k], (name, cut, off, ln)
    assert cb.lib().inflcut_bad_loads() == 0


@pytest.mark.parametrize("cut", cc.CUT_BYTES)
@pytest.mark.parametrize("name", ["text/w0", "stored/w0", "fixed/w2", "hand/w0"])
def test_the_block_counts_of_the_cuts_sum_to_the_entries(name, cut):
    c = cc.by_name(name)
    n = len(c.want)
    keys = ("n_blocks", "n_stored", "n_fixed", "n_dynamic")
    whole0 = build(c, 0).read(0, n)
    whole = build(c, cut).read(0, n)
    # a read to the end decodes every cut but those behind the stream's last byte (empty blocks at the end of the last entry): a
    # block's kind is counted by the cut that holds its header, the block by the cut that holds its end
    cl, _on = cc.cuts(c, cut)
    places, _m, end = cc.walk(c.raw, tuple(c.table))
    first_of_last = max(i for i, x in enumerate(cl) if x[0] == c.table[-1][0])
    undecoded = [x for i, x in enumerate(cl) if i > first_of_last and x[1] >= n]
    stop = undecoded[0][0] if undecoded else end[0]
    hdrs = [pl for pl in places if pl.kind[0] == "H"]
    ends = [h.bit for h in hdrs[1:]] + [end[0]]
    want = [sum(1 for e in ends if e <= stop)] + [sum(1 for h in hdrs if h.bit < stop and h.kind == k) for k in ("H0", "H1", "H2")]
    assert whole[0] == cb.OK and [whole[2][k] for k in keys] == want, (whole[2], want)
    assert whole[6]["cuts"] == len(cl) - len(undecoded)
    if not undecoded:
        assert want == [whole0[2][k] for k in keys]  # the sums over every entry's cuts are the entries'


@pytest.mark.parametrize("name", ["text/w0", "fixed/w0", "hand/w0"])
def test_a_range_in_pieces_and_batches_that_share_a_set(name):
    c = cc.by_name(name)
    ix = build(c, 256, group=cb.GROUP_MIN)
    ranges = [cc.LONG, (0, len(c.want)), (len(c.want) // 2, 70000)]
    rc, res, counts, cuts = ix.read_batch(ranges, group=cb.GROUP_MIN)
    assert rc == cb.OK and cuts["launches"] == 4 * counts["sets"]
    if len(cc.points(c)) > 1:
        assert counts["sets"] >= 3
    check(c, ranges, res, "pieces")
    ix = build(c, 256)
    for ranges in cc.batches(c, 256):
        rc, res, counts, cuts = ix.read_batch(ranges)
        assert rc == cb.OK and counts["sets"] == 1 and cuts["launches"] == 4
        check(c, ranges, res, "batch of %d" % len(ranges))
        assert [ix.read(off, ln)[:5] for off, ln in ranges] == res


@pytest.mark.parametrize("name", ["text/w0", "hand/w0"])
def test_damage_after_the_build_is_rejected_where_a_cut_decodes_it(name):
    c = cc.by_name(name)
    cut = 256
    ix = build(c, cut)
    (off, ln), flips, hdr = cc.damage(c, cut)
    failed = {"header": 0, "token": 0, "outside": 0}
    statuses = set()
    for kind, bit in flips:
        rc, got, rep, buf, canary, _counts, _cuts = ix.read(off, ln, stream=cc.flipped(c.stream, bit))
        assert canary
        if kind == "outside":
            assert (rc, got, buf) == (cb.OK, ln, c.want[off:off + ln]), (kind, bit, rep)
            continue
        if rc == cb.E_DATA:
            failed[kind] += 1
            statuses.add(rep["status"])
            assert rep["status"] != "OK" and got == min(max(rep["out_pos"], off) - off, ln) and rep["out_len"] == 0, (kind, bit, rep)
            assert buf[:got] == c.want[off:off + got]
            if kind == "header":  # reported at the header, by the cut that stands on it or the first one inside its block
                assert hdr <= rep["bit"] <= bit + 400 and rep["out_pos"] < off and got == 0, (bit, rep)
        else:
            assert got == ln  # (a flip that leaves every cut ending where its successor begins is not noticed: no checksum on a read)
        assert buf[got:] == FILL * (ln - got), (kind, bit)
        rc2, res, _c, _s = ix.read_batch([(off, ln), (0, 100)], stream=cc.flipped(c.stream, bit))
        assert res[0][:4] == (rc, got, rep, buf) and res[1][0] == cb.OK and res[1][3] == c.want[:100] and rc2 == rc
    assert failed["header"] >= 1 and failed["token"] >= 1 and failed["outside"] == 0, failed
    assert "TABLE" in statuses, statuses  # a cut that runs past its successor
    # a stream cut short (the same length, zeros behind the cut): a read that reaches the zeros fails, one in front of them does not
    short = c.stream[:len(c.stream) * 3 // 4] + bytes(len(c.stream) - len(c.stream) * 3 // 4)
    rc, got, rep, buf, canary, _counts, _cuts = ix.read(len(c.want) - 5000, 5000, stream=short)
    assert rc == cb.E_DATA and canary and buf[got:] == FILL * (5000 - got)
    assert ix.read(10, 100, stream=short)[:2] == (cb.OK, 100)


@pytest.mark.parametrize("name", ["text/w0", "hand/w0", "fixed/w0"])
def test_a_mutated_cut_list_never_gives_wrong_bytes_with_ok(name):
    c = cc.by_name(name)
    cut = 256
    want, on = cc.cuts(c, cut)
    token = [i for i, x in enumerate(want) if x[0] != x[2]]
    hdrs = sorted({x[2] for x in want})
    n, caught = len(c.want), 0
    for i in token[1::max(len(token) // 6, 1)]:
        bit, pos, hdr = want[i]
        other = [h for h in hdrs if h != hdr]
        muts = [(bit + 1, pos, hdr), (bit - 1, pos, hdr), (bit, pos + 1, hdr), (bit, pos, hdr + 1)] + [(bit, pos, h) for h in other[:2]]
        for m in muts:
            ix = build(c, cut)
            ix.set_cut(i, m)
            lo = max(pos - 2000, 0)
            rc, got, rep, buf, canary, _counts, _cuts = ix.read(lo, 4000)
            assert canary and buf[:got] == c.want[lo:lo + got] and buf[got:] == FILL * (4000 - got), (name, i, m, rep)
            if rc == cb.OK:
                assert got == min(4000, n - lo)
            else:
                caught += 1
                assert rep["status"] in ("TABLE", "BTYPE", "LENGTHS", "CODE", "DISTANCE", "TRUNCATED", "STORED"), (name, i, m, rep)
    assert caught >= 6, caught


def test_the_mutants_die():
    c = cc.by_name("text/w0")
    # the rule measured from the entry's start: another cut list, and more cuts than the entry has slots
    ix = build(c, 256, mutant=cb.MUTANT_RULE)
    assert ix.cuts() != cc.cuts(c, 256)[0] and ix.info()["surplus"] > 0
    # flatten's inside test off by one: a match of a later cut that copies the entry's first byte
    c = cc.by_name("hand/w0")
    hit = 0
    for name, mutant in (("hand/w0", cb.MUTANT_INSIDE), ("text/w0", cb.MUTANT_INSIDE)):
        c = cc.by_name(name)
        ix, good = build(c, 64, mutant=mutant), build(c, 64)
        rc, got, _rep, buf, _canary, _c, _s = ix.read(0, len(c.want))
        assert good.read(0, len(c.want))[3] == c.want
        hit += (rc, buf) != (cb.OK, c.want)
    assert hit >= 1
    # the stop test without the position: a cut list whose positions are one off stops all the same
    c = cc.by_name("text/w0")
    want, _on = cc.cuts(c, 256)
    i = [k for k, x in enumerate(want) if x[0] != x[2]][5]
    bit, pos, hdr = want[i]
    lo = max(pos - 2000, 0)
    good, bad = build(c, 256), build(c, 256, mutant=cb.MUTANT_STOP)
    good.set_cut(i, (bit, pos + 1, hdr))
    bad.set_cut(i, (bit, pos + 1, hdr))
    assert good.read(lo, 4000)[2]["status"] == "TABLE"
    r = bad.read(lo, 4000)
    assert (r[0], r[2]["bit"]) != (good.read(lo, 4000)[0], good.read(lo, 4000)[2]["bit"]) or r[3] != good.read(lo, 4000)[3]


def test_the_standalone_sanitizer_program_runs_clean(tmp_path):
    cases = []
    for c in cc.corpus():
        for cut in cc.CUT_BYTES:
            if c.wrapper and cut != 256:
                continue
            cases.append((c.stream, c.wrapper, c.table, cc.SPACING, cb.GROUP_DEFAULT, cut, c.want, cc.ranges(c, cut, every=False)[::5], None))
    c = cc.by_name("text/w0")
    cases.append((c.stream, 0, c.table, cc.SPACING, cb.GROUP_MIN, 64, c.want, [cc.LONG, (0, len(c.want))], None))
    for name in ("text/w0", "hand/w0"):
        c = cc.by_name(name)
        (off, ln), flips, _hdr = cc.damage(c, 256)
        for _kind, bit in flips:
            cases.append((c.stream, 0, c.table, cc.SPACING, cb.GROUP_MIN, 256, c.want, [(off, ln), (1000, 100000)], cc.flipped(c.stream, bit)))
    cases.append((c.stream[:-100] + bytes(100), 0, c.table, cc.SPACING, cb.GROUP_DEFAULT, 256, c.want, [(0, 10)], None))  # (no index)
    path = os.path.join(str(tmp_path), "corpus.bin")
    cb.write_corpus(path, cases)
    status, out = cb.run_fuzz(path)
    assert status == 0, out
    assert "%d cases" % len(cases) in out and " 2 refused" in out
