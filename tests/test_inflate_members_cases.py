"""The members inflate (deflate-rs_amd/csrc/inflate_members.h) as the host build of tests/inflmembers runs it over the cases of
inflate_members_cases.py: the serial walk agrees with zlib on every file, in both directions; the call as the device runs it --
Path A over the hinted runs, Path B over the rest -- equals the serial walk in return value, length, report, member table and the
bytes that hold data at four span sizes, with the canary behind out_cap whole; a file of one member equals the one-wave inflate;
every precondition a case is named for is asserted here, so that a case cannot silently stop forcing its edge; and every mutant of
the model is caught.  CPU only."""
import os
import zlib

import pytest

import inflate_members_cases as mc
import inflmembers_binding as mb
import inflwrite_binding as wb

CASES = mc.corpus()
IDS = [c.name for c in CASES]


def spans():
    return [16, 64, 4096, mb.span_default()]


def own_cap(c):
    """the buffer a case is given: zlib's length; for a refused file the exact size if it is structurally valid (so that its
    checksums are judged), else 1000 bytes"""
    if c.want is not None:
        return len(c.want)
    rc, n, _rep, _m, _d, _ok = mb.serial(c.stream, 0)
    return n if rc == mb.E_OUT_TOO_SMALL else 1000


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: the serial walk and both finders have run under ASan + UBSan, with exact-size file, output and table
    allocations, before anything else"""
    cases = []
    for c in CASES:
        for S in spans():
            cases.append((c.stream, S, own_cap(c)))
        for cap in c.caps:
            cases.append((c.stream, 16, cap))
    path = os.path.join(str(tmp_path), "corpus.bin")
    mb.write_corpus(path, cases)
    rc, out = mb.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_serial_walk_agrees_with_zlib(c):
    rc, n, rep, members, data, ok = mb.serial(c.stream, own_cap(c))
    assert ok
    if c.want is not None:
        assert (rc, n, data, rep["status"]) == (mb.OK, len(c.want), c.want, "OK"), rep
        assert [m[3] for m in members] == [len(x) for x in mc.zlib_members(c.stream)]
        assert sum(m[1] for m in members) == len(c.stream) and all(m[5] == "OK" for m in members)
    else:
        assert rc == mb.E_DATA and rep["status"] != "OK" and members[-1][5] == rep["status"], rep
        assert n == min(rep["out_pos"], own_cap(c))
        # what was decoded in front of the failure is what zlib decodes in front of its error
        for m in members[:-1]:
            if m[2] + m[3] <= n:
                assert zlib.decompressobj(31).decompress(c.stream[m[0]: m[0] + m[1]]) == data[m[2]: m[2] + m[3]]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_paths_equal_the_serial_walk(c):
    for cap in (own_cap(c),) + c.caps:
        want = mb.structure(mb.serial(c.stream, cap))
        assert want[5]
        for S in spans():
            got = mb.run(c.stream, S, cap)
            assert mb.structure(got) == want, (c.name, S, cap, got[:3], want[:3])
            assert mb.structure(mb.run(c.stream, S, cap, lanes=False)) == want, (c.name, S, cap)
            # HINTED only where the member does state its size, truly
            for m in got[3]:
                if m[4] & mb.HINTED:
                    assert mb.hint(c.stream, m[0])[:3] == (True, True, m[1]) and m[5] in ("OK", "CHECKSUM")


def test_short_buffers_and_the_size_query():
    n_caps = 0
    for c in CASES:
        if c.want is None or not c.caps:
            continue
        for cap in c.caps:
            rc, n, rep, members, data, ok = mb.run(c.stream, 64, cap)
            n_caps += 1
            assert ok and data == c.want[:cap]
            assert (rc, n) == (mb.OK if cap >= len(c.want) else mb.E_OUT_TOO_SMALL, len(c.want)), (c.name, cap)
            assert len(members) == len(mc.zlib_members(c.stream)) and rep["out_len"] == len(c.want)
    assert n_caps > 60


SINGLE = [c for c in CASES if c.name.startswith("single/")]


@pytest.mark.parametrize("c", SINGLE, ids=[c.name for c in SINGLE])
def test_a_file_of_one_member_equals_the_one_wave_inflate(c):
    for cap in {own_cap(c), 0, 7}:
        ref = wb.inflate(c.stream, 2, cap)
        got = mb.run(c.stream, 64, cap)
        if c.name in ("single/gzip_byte_behind", "single/gzip_second_member"):
            # the one exception: bytes behind the trailer are TRAILER there and the next member here
            assert ref[2]["status"] == "TRAILER"
            if cap == own_cap(c):
                assert got[2]["status"] == ("FRAME" if "byte" in c.name else "OK")
            continue
        assert (got[0], got[1], got[2]) == ref[:3], (c.name, cap, got[:3], ref[:3])
        assert got[4] == ref[3][:min(ref[1], cap)] and got[5]


# ---- preconditions of the named cases -----------------------------------------------------------------------------------------------
def smallest_hinted(stream, S):
    """the definition of a span's candidate: the smallest hinted offset in it"""
    out = [mb.NOCAND] * mb.n_spans(len(stream), S)
    for o in range(len(stream) - 1, -1, -1):
        if mb.hint(stream, o)[0]:
            out[o // S] = o
    return out


def test_finder_finds_the_smallest_hinted_offset_of_every_span():
    for name in ("bgzf/every_residue", "bgzf/n130", "decoy/shadow", "decoy/stored_bgzf_file", "mixed/alternating_11", "liar/bsize+1"):
        c = mc.by_name(name)
        for S in (16, 64, 4096):
            want = smallest_hinted(c.stream, S)
            assert mb.scan(c.stream, S)[0] == want == mb.scan(c.stream, S, lanes=False)[0], (name, S)


def test_prefilter_spares_the_full_test():
    c = mc.by_name("bgzf/blocks")
    mb.reset_counters()
    mb.scan(c.stream, 4096)
    cnt = mb.counters()
    # (a span is left at its first hinted offset; only the four fixed bytes of a member start pass the prefilter in this file)
    assert len(c.stream) // 2 < cnt["offsets"] <= len(c.stream) and 1 <= cnt["parses"] <= c.facts["n_parts"], cnt


def test_preconditions_of_the_bgzf_cases():
    c = mc.by_name("bgzf/every_residue")
    st = c.facts["starts"]
    assert {o % 64 for o in st} == set(range(64)) and st[0] % 64 == 0 and any(o and o % 64 == 0 for o in st)
    assert all(mb.hint(c.stream, o)[0] for o in st)
    for S in (16, 64):
        rc, _n, _rep, members, _d, _ok = mb.run(c.stream, S, len(c.want))
        assert rc == mb.OK and all(m[4] & mb.HINTED for m in members) and [m[0] for m in members] == st
        cand, walks = mb.scan(c.stream, S)
        sizes = [b - a for a, b in zip(st, st[1:])]
        assert max(sizes) > S and mb.NOCAND in cand  # a member larger than a span, a span with no start
    c = mc.by_name("bgzf/blocks")
    sizes = [len(x) for x in mc.zlib_members(c.stream)]
    assert sizes == [0, 1, 63, 64, 65, 0xff00, 0] and c.stream.endswith(mc.BGZF_EOF) and len(mc.BGZF_EOF) == 28
    assert max(b - a for a, b in zip(c.facts["starts"], c.facts["starts"][1:])) > 4096
    for name, n in (("bgzf/n1", 1), ("bgzf/n2", 2), ("bgzf/n65", 65), ("bgzf/n130", 130)):
        members = mb.run(mc.by_name(name).stream, 64, len(mc.by_name(name).want))[3]
        assert len(members) == n and all(m[4] & mb.HINTED for m in members)
    # the first BC subfield of length 2 counts; one of another length in front of it is skipped
    c = mc.by_name("bgzf/bc_behind_a_subfield")
    assert all(mb.hint(c.stream, o)[0] for o in c.facts["starts"])
    c = mc.by_name("bgzf/bc_in_front_of_a_subfield")
    assert all(mb.hint(c.stream, o)[0] for o in c.facts["starts"])
    for name in ("plain/headers", "plain/17", "plain/oracle_arena"):
        c = mc.by_name(name)
        assert not any(m[4] for m in mb.run(c.stream, 64, len(c.want))[3])
        assert mb.scan(c.stream, 64)[0] == [mb.NOCAND] * mb.n_spans(len(c.stream), 64)
    c = mc.by_name("plain/headers")
    assert {c.stream[o + 3] for o in c.facts["starts"]} == {8, 2 | 4 | 8 | 16, 0}  # FNAME; FHCRC FEXTRA FNAME FCOMMENT; none


def test_mixed_files_resume_path_a_and_cross_the_resume_bound():
    c = mc.by_name("mixed/hinted_plain_hinted")
    members = mb.run(c.stream, 64, len(c.want))[3]
    assert [m[4] & mb.HINTED for m in members] == [1, 1, 1, 0, 0, 1, 1, 1, 1]
    c = mc.by_name("mixed/plain_then_hinted")
    assert [m[4] & mb.HINTED for m in mb.run(c.stream, 64, len(c.want))[3]] == [0, 0, 1, 1, 1, 1, 1]
    c = mc.by_name("mixed/alternating_11")
    assert c.facts["alternations"] > mb.lib().inflmembers_resumes() == 8
    mb.reset_counters()
    rc, _n, _rep, members, data, _ok = mb.run(c.stream, 64, len(c.want))
    cnt = mb.counters()
    flags = [m[4] & mb.HINTED for m in members]
    assert rc == mb.OK and data == c.want
    assert flags == [0, 1, 1] * 8 + [0] * 9  # eight resumes, then the hints are ignored
    assert cnt["runs"] == 9 and cnt["chains"] == 9, cnt  # the first attempt and eight resumes; one launch of Path B between them


def test_groups_and_rooms_of_one_member_change_nothing():
    try:
        mb.set_rooms(1, 1)
        for name in ("bgzf/n65", "mixed/alternating_11", "plain/17", "liar/bsize-1", "damage/bgzf/middle/data"):
            c = mc.by_name(name)
            cap = own_cap(c)
            assert mb.structure(mb.run(c.stream, 64, cap)) == mb.structure(mb.serial(c.stream, cap)), name
        mb.reset_counters()
        c = mc.by_name("plain/17")
        mb.run(c.stream, 64, 0)
        assert mb.counters()["chains"] == 17
    finally:
        mb.set_rooms(0, 0)


def test_decoys():
    c = mc.by_name("decoy/stored_bgzf_file")
    inner_at = c.facts["starts"][2] + 15
    assert mb.hint(c.stream, inner_at)[0] and c.stream[c.facts["starts"][2] + 3] == 0  # a hinted header in a plain member's payload
    assert [m[4] & mb.HINTED for m in mb.run(c.stream, 64, len(c.want))[3]] == [1, 1, 0, 1, 1, 1, 1]
    # the decoy is its span's candidate, the true start behind it in the same span is shadowed -- and still decoded as hinted
    c = mc.by_name("decoy/shadow")
    d, t = c.facts["decoy"], c.facts["true"]
    assert d // 64 == t // 64 >= 1 and d < t and t == c.facts["starts"][2]
    assert mb.hint(c.stream, d)[:3] == (True, True, 30) and mb.hint(c.stream, t)[0]
    cand, walks = mb.scan(c.stream, 64)
    assert cand[d // 64] == d and t not in cand
    w = walks[d // 64]
    assert (w[0], w[2], mb.HOW[w[4]]) == (d, 1, "open")  # the decoy's walker hops once and stands on nothing
    rc, _n, _rep, members, data, _ok = mb.run(c.stream, 64, len(c.want))
    assert rc == mb.OK and data == c.want and all(m[4] & mb.HINTED for m in members) and [m[0] for m in members] == c.facts["starts"]
    # the decoy's claimed extent ends exactly on a true start that is its span's candidate: its walker links into the true chain
    c = mc.by_name("decoy/lands_on_a_true_start")
    d, t = c.facts["decoy"], c.facts["true"]
    assert t == c.facts["starts"][2] and d // 64 < t // 64
    cand, walks = mb.scan(c.stream, 64)
    assert cand[d // 64] == d and cand[t // 64] == t
    w = walks[d // 64]
    assert (w[1], w[2], mb.HOW[w[4]], w[5]) == (t, 1, "link", t // 64)
    rc, _n, _rep, members, data, _ok = mb.run(c.stream, 64, len(c.want))
    assert rc == mb.OK and data == c.want and [m[0] for m in members] == c.facts["starts"] and all(m[4] & mb.HINTED for m in members)


def test_lying_hints_are_judged_by_the_serial_walk():
    for name, valid in (("liar/bsize+1", True), ("liar/bsize-1", True), ("liar/bsize_past_the_end", True), ("liar/bsize_first_member", True),
                        ("liar/bsize_spans_two_members", True), ("damage/bgzf/bsize_field", True), ("liar/isize_too_small", False),
                        ("liar/isize_too_large", False), ("liar/isize_plain_member", False)):
        c = mc.by_name(name)
        assert (c.want is not None) == valid, name
        liar = 0 if "first" in name else 1 if "spans_two" in name or "plain_member" in name else 4 if "past" in name else 2
        o = c.facts["starts"][liar] if c.facts["n_parts"] > 1 else None
        rc, _n, rep, members, _d, _ok = mb.run(c.stream, 64, own_cap(c))
        if valid:
            assert rc == mb.OK
            if o is not None:
                m = [m for m in members if m[0] == o][0]
                assert not m[4] & mb.HINTED, name  # the member whose hint lies was walked by Path B
        else:
            assert (rc, rep["status"]) == (mb.E_DATA, "CHECKSUM") and len(members) == liar + 1 and members[-1][5] == "CHECKSUM"
    # a false ISIZE: CHECKSUM once the member is stored whole, the exact size below that
    for name in ("liar/isize_too_small", "liar/isize_too_large"):
        c = mc.by_name(name)
        at, total = c.facts["at"], c.facts["total"]
        for cap in c.caps:
            rc, n, rep, _m, _d, _ok = mb.run(c.stream, 64, cap)
            if cap >= total:
                assert (rc, rep["status"], rep["out_pos"], n) == (mb.E_DATA, "CHECKSUM", at, at), (name, cap)
            else:
                assert (rc, n) == (mb.E_OUT_TOO_SMALL, total), (name, cap)
    # a structural failure behind it: the member that was stored whole is judged first, one that was not is not
    c = mc.by_name("liar/isize_too_small")
    cut = c.stream[:-20]
    at = c.facts["at"]
    assert mb.run(cut, 64, at)[2]["status"] == "CHECKSUM" and mb.run(cut, 64, at - 1)[2]["status"] == "TRUNCATED"
    assert mb.structure(mb.run(cut, 64, at - 1)) == mb.structure(mb.serial(cut, at - 1))


def test_damage_is_reported_in_file_order():
    seen = set()
    for c in CASES:
        if not c.name.startswith("damage/"):
            continue
        rc, _n, rep, members, _d, _ok = mb.run(c.stream, 64, own_cap(c))
        seen.add(rep["status"])
        if "damaged" in c.facts and rc == mb.E_DATA:
            assert len(members) == c.facts["damaged"] + 1, c.name
        if c.name.endswith("trailing_zeros") or c.name.endswith("one_trailing_byte"):
            assert (rc, rep["status"], rep["bit"], len(members)) == (mb.E_DATA, "FRAME", 0, 6) and rep["out_pos"] == members[-1][2]
    assert {"OK", "FRAME", "TRUNCATED", "CHECKSUM"} <= seen and len(seen) >= 6, seen
    c = mc.by_name("damage/empty_file")
    assert mb.run(c.stream, 64, 0)[:4] == mb.serial(c.stream, 0)[:4]
    assert mb.serial(c.stream, 0)[2]["status"] == "FRAME" and mb.serial(c.stream, 0)[3] == [(0, 0, 0, 0, 0, "FRAME")]


# ---- mutants of the model: each is caught by a named case ---------------------------------------------------------------------------------
def test_mutant_last_candidate_is_caught_by_two_starts_in_a_span():
    c = mc.by_name("bgzf/n130")
    assert mb.scan(c.stream, 4096)[0] == smallest_hinted(c.stream, 4096)
    assert mb.scan(c.stream, 4096, mutant=mb.MUTANT_LAST_CANDIDATE)[0] != smallest_hinted(c.stream, 4096)
    # with a decoy BEHIND the true start of a span the last candidate is the decoy: the link is missed, never a byte
    c = mc.by_name("decoy/lands_on_a_true_start")
    got = mb.run(c.stream, 4096, len(c.want), mutant=mb.MUTANT_LAST_CANDIDATE)
    assert mb.structure(got) == mb.structure(mb.serial(c.stream, len(c.want)))


def test_mutant_stop_at_or_beyond_the_candidate_is_caught_by_the_shadowing_decoy():
    c = mc.by_name("decoy/shadow")
    good = mb.run(c.stream, 64, len(c.want))
    bad = mb.run(c.stream, 64, len(c.want), mutant=mb.MUTANT_STOP_GE)
    assert bad != good and mb.scan(c.stream, 64, mutant=mb.MUTANT_STOP_GE)[1] != mb.scan(c.stream, 64)[1]
    # the walker that stood on the true start linked to the decoy's span: the run was cut there and the true member left to Path B
    t = c.facts["true"]
    assert [m[4] & mb.HINTED for m in bad[3] if m[0] == t] == [0] and [m[4] & mb.HINTED for m in good[3] if m[0] == t] == [1]
    assert mb.structure(bad) == mb.structure(good)  # ... which costs time and never a byte


def test_mutant_total_is_bsize_is_caught_by_every_bgzf_file():
    c = mc.by_name("bgzf/n65")
    good = mb.run(c.stream, 64, len(c.want))
    bad = mb.run(c.stream, 64, len(c.want), mutant=mb.MUTANT_TOTAL_IS_BSIZE)
    assert all(m[4] & mb.HINTED for m in good[3]) and not any(m[4] & mb.HINTED for m in bad[3])
    assert mb.hint(c.stream, 0)[2] == c.facts["starts"][1]
    assert mb.structure(bad) == mb.structure(good)
