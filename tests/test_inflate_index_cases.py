"""The inflate index (deflate-rs_amd/csrc/inflate_index.h) as the host build of tests/inflindex runs it over the cases of
inflate_index_cases.py: the finder with its prefilter finds what the plain predicate finds; every known non-final dynamic block start
passes the predicate; the table's entries are true block starts, the tabled host build accepts it and its bytes are zlib's; where no
false candidate exists the table has one entry per span with a true start; and the combined call equals the one-wave inflate of
tests/inflwrite in return value, length, report and bytes on every stream, damaged ones and short buffers included.  Every
precondition a case is named for is asserted here, so that a case cannot silently stop forcing its edge.  CPU only."""
import os

import pytest

import inflate_cases as icases
import inflate_index_cases as xc
import inflate_table_cases as tc
import inflindex_binding as xb
import infltable_binding as tb
import inflwrite_binding as wb

STREAMS = xc.streams()
IDS = [c.name for c in STREAMS]


def spans():
    return [256, 4096, xb.span_default()]


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: finder, walkers, link and the combined call have run under ASan + UBSan, with exact-size stream, candidate
    and record arrays, before anything else"""
    cases = []
    for c in STREAMS:
        cap = len(c.want) if c.want is not None else 1000
        for S in spans():
            cases.append((c.stream, c.wrapper, cap, S, xb.GROUP_DEFAULT))
        cases.append((c.stream, c.wrapper, cap // 2, 256, tc.GROUP_MIN))
    for c in xc.mutated(links_256())[::3] + list(icases.rejected())[::4]:
        cases.append((c.stream, c.wrapper, 20000, 256, xb.GROUP_DEFAULT))
    path = os.path.join(str(tmp_path), "corpus.bin")
    xb.write_corpus(path, cases)
    rc, out = xb.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


def by_name(name):
    return xc.by_name(name)


def true_starts(c):
    """every non-final dynamic block start of the stream's serial walk (the host build's block list)"""
    return [b for b, h in xb.blocks(c.stream, c.wrapper) if h == 4]


def links_256():
    """[(first bit, end bit)] of the mutation base's entries at S = 256"""
    c = by_name(xc.MUTATION_BASE)
    rc, _n, table, _spans, _rep = xb.index(c.stream, 0, 256)
    assert rc == xb.OK and len(table) >= 3  # a first, a middle and a last link
    bits = [t["bit_start"] for t in table] + [8 * len(c.stream)]
    return [(bits[k], bits[k + 1]) for k in range(len(table))]


def same_as_inflate(c, S, cap, **kw):
    got = xb.parallel(c.stream, c.wrapper, S, cap, **kw)
    ref = wb.inflate(c.stream, c.wrapper, cap)
    assert got[:3] == ref[:3], (c.name, S, cap, got[:3], ref[:3])
    assert got[3] == ref[3], (c.name, S, cap)
    assert got[4] and ref[4], (c.name, S, cap)
    return got


# ---- the finder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", STREAMS, ids=IDS)
def test_prefiltered_finder_equals_the_plain_predicate(c):
    for S in spans():
        assert xb.scan(c.stream, c.wrapper, S, lanes=True) == xb.scan(c.stream, c.wrapper, S, lanes=False), S


def test_prefilter_spares_the_full_parse():
    c = by_name("text/l6")
    xb.reset_counters()
    xb.scan(c.stream, 0, xb.span_default())
    cnt = xb.counters()
    # on random bits the three header bits pass one offset in 8, and the Kraft sum, whatever the other lengths are, allows the last
    # length one value in 8: one full parse in 64 offsets; twice that is allowed for bits that are not random
    assert cnt["offsets"] > len(c.stream) and cnt["parses"] * 32 < cnt["offsets"], cnt


@pytest.mark.parametrize("c", STREAMS, ids=IDS)
def test_known_block_starts_pass_the_predicate(c):
    known = set(c.starts or [])
    walked = set(true_starts(c))
    assert known <= walked
    if c.complete:
        assert known == walked
    for b in walked:
        assert xb.is_start(c.stream, c.wrapper, b) == (True, True), b
    # ... and at S = 256 a span that holds one has a candidate at or in front of it
    cand, _recs = xb.scan(c.stream, c.wrapper, 256)
    for b in walked:
        k = b // 2048
        assert cand[k] != xb.NOCAND and cand[k] <= b and (k == 0 or cand[k] // 2048 == k)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", STREAMS, ids=IDS)
def test_table_is_the_serial_walk(c):
    starts = {b for b, _h in xb.blocks(c.stream, c.wrapper)}
    heads = dict(xb.blocks(c.stream, c.wrapper))
    for S in spans():
        rc, n, table, chain, rep = xb.index(c.stream, c.wrapper, S)
        assert n == len(table) >= 1 and n <= xb.n_spans(len(c.stream), S)
        assert table[0]["bit_start"] == 0 and chain[0] == 0
        assert all(t["n_tokens"] == 0 and t["reserved"] == 0 for t in table)
        pairs = [(t["bit_start"], t["in_bytes"]) for t in table]
        if c.want is None:
            assert rc == xb.E_DATA and rep["status"] != "OK" and rep["out_pos"] == sum(nb for _b, nb in pairs)
            assert all(t["bfinal"] == 0 for t in table)
            good = table[:-1]
        else:
            assert rc == xb.OK and rep["status"] == "OK" and rep["out_len"] == len(c.want) == sum(nb for _b, nb in pairs)
            assert [t["bfinal"] for t in table] == [0] * (n - 1) + [1]
            good = table
            # the judge: the tabled host build takes the table as it stands, and the bytes are zlib's
            trc, tn, trep, buf, ok = tb.inflate(c.stream, c.wrapper, pairs, len(c.want))
            assert (trc, tn, buf, ok) == (tb.OK, len(c.want), c.want, True), (S, trep)
            assert {k: rep[k] for k in ("n_blocks", "n_stored", "n_fixed", "n_dynamic")} == \
                   {k: trep[k] for k in ("n_blocks", "n_stored", "n_fixed", "n_dynamic")}
        for t in good:
            assert t["bit_start"] in starts and t["btype"] == heads[t["bit_start"]] >> 1, (S, t)


DECOY_FREE = [c for c in STREAMS if c.want is not None and not c.name.startswith("decoy/")]


@pytest.mark.parametrize("c", DECOY_FREE, ids=[c.name for c in DECOY_FREE])
def test_one_entry_per_span_with_a_true_start(c):
    true = set(true_starts(c))
    for S in spans():
        cand, _recs = xb.scan(c.stream, c.wrapper, S)
        # these seeds have no false candidate (one that had would have to be replaced, not excused)
        assert [b for b in cand[1:] if b != xb.NOCAND and b not in true] == [], S
        _rc, n, _table, _chain, _rep = xb.index(c.stream, c.wrapper, S)
        assert n == 1 + len({b // (8 * S) for b in true if b >= 8 * S}), S


# ---- preconditions of the named cases ---------------------------------------------------------------------------------------------------
def test_preconditions_of_the_streams():
    for level in (1, 6, 9):
        c = by_name("text/l%d" % level)
        assert len(c.want) == 1 << 20 and xb.index(c.stream, 0, xb.span_default())[1] >= 5
    for c in STREAMS:
        assert c.want is None or len(c.want) <= (1 << 20) + 4096, c.name
    # the cut stream: an empty stored block in front of every entry but the first, their fronts on all 8 bit phases
    c = by_name("zcut/phases")
    bl = xb.blocks(c.stream, 0)
    fronts = [b for (b, h), (b2, _h2) in zip(bl, bl[1:]) if h == 0 and b2 in c.facts["entries"]]
    assert len(fronts) == len(c.facts["entries"]) - 1 and {b % 8 for b in fronts} == set(range(8))
    assert len(bl) == 2 * len(c.facts["entries"]) - 1  # (an entry is one block and the flush's)
    # dynamic block starts on all 8 phases, every one the candidate of its span
    c = by_name("hand/phases")
    cand, _recs = xb.scan(c.stream, 0, 256)
    assert {b % 8 for b in c.starts} == set(range(8)) and set(c.starts) <= set(cand)
    # first bit of a span, last bit of a span, a header across a span edge
    c = by_name("hand/span_edges")
    cand, _recs = xb.scan(c.stream, 0, 256)
    s1, s2, s3 = c.starts
    assert (s1 % 2048, s2 % 2048) == (0, 2047) and cand[s1 // 2048] == s1 and cand[s2 // 2048] == s2
    assert s3 // 2048 != (s3 + 57) // 2048 and cand[s3 // 2048] == s3  # (17 + 3 x 19 bits of the header at least lie across)
    assert [b for b in cand if b != xb.NOCAND] == [0, s1, s2, s3]
    # a header across the end of the stream is no candidate, and the stream is TRUNCATED
    c = by_name("hand/header_across_the_end")
    h = c.facts["header"]
    assert 8 * len(c.stream) - 57 < h + 17 < 8 * len(c.stream) and xb.is_start(c.stream, 0, h)[0] is False
    cand, _recs = xb.scan(c.stream, 0, 256)
    assert cand[h // 2048] == xb.NOCAND
    rc, _n, _table, _chain, rep = xb.index(c.stream, 0, 256)
    assert rc == xb.E_DATA and rep["status"] == "TRUNCATED"
    full = by_name("hand/phases")
    assert xb.is_start(full.stream, 0, h) == (True, True)
    # one entry whatever the span: fixed only (several blocks), stored only (several pieces of 65 535 bytes), a megabyte of zeros
    for name, key, least in (("fixed", "n_fixed", 2), ("stored", "n_stored", 4), ("zeros_1m", "n_dynamic", 1)):
        c = by_name(name)
        for S in spans():
            rc, n, table, _chain, rep = xb.index(c.stream, 0, S)
            assert (rc, n) == (xb.OK, 1) and rep[key] == rep["n_blocks"] >= least, (name, S)
    assert len(by_name("zeros_1m").stream) > 256 * 3  # (several spans of 256 all the same)
    for name in ("huffman_only", "rle", "zlib", "gzip_name_extra"):
        c = by_name(name)
        assert xb.index(c.stream, c.wrapper, 256)[1] >= 2, name
    assert by_name("gzip_name_extra").stream[3] & (4 | 8) == 4 | 8  # FEXTRA and FNAME
    for name in ("empty", "one_byte"):
        c = by_name(name)
        assert len(c.stream) == ("empty", "one_byte").index(name) and xb.index(c.stream, 0, 256)[4]["status"] == "TRUNCATED"


def test_decoy_in_front_of_a_true_boundary_is_not_on_the_chain():
    c = by_name("decoy/a")
    decoy, d, e = c.facts["decoy"], c.facts["d"], c.facts["e"]
    assert decoy % 8 == 0 and xb.is_start(c.stream, 0, decoy) == (True, True)
    assert decoy // 2048 == d // 2048 == 1 and decoy < d  # the decoy and the true boundary in one span, the decoy first
    cand, recs = xb.scan(c.stream, 0, 256)
    assert cand[1] == decoy and d not in cand  # the true boundary is shadowed
    w = xb.Walk(*recs[1])
    assert xb.HOW[w.how] == "failed" and xb.STATUS[w.status] == "BTYPE" and w.n_blocks == 0  # the decoy block, then BTYPE 3
    rc, n, table, chain, _rep = xb.index(c.stream, 0, 256)
    assert rc == xb.OK and 1 not in chain and [t["bit_start"] for t in table] == [0, e]
    for S in spans():
        assert same_as_inflate(c, S, len(c.want))[3] == c.want


def test_decoy_that_links_to_a_true_candidate_is_ignored():
    c = by_name("decoy/b")
    decoy, d = c.facts["decoy"], c.facts["d"]
    assert xb.is_start(c.stream, 0, decoy) == (True, True) and decoy // 2048 == 1 and d // 2048 == 2
    cand, recs = xb.scan(c.stream, 0, 256)
    assert cand[1] == decoy and cand[2] == d
    w = xb.Walk(*recs[1])
    assert xb.HOW[w.how] == "link" and w.link == 2 and w.end_bit == d  # the decoy ends exactly where the stored block ends
    rc, n, table, chain, _rep = xb.index(c.stream, 0, 256)
    assert rc == xb.OK and chain == [0, 2] and [t["bit_start"] for t in table] == [0, d]
    for S in spans():
        assert same_as_inflate(c, S, len(c.want))[3] == c.want


# ---- the combined call against the one-wave inflate -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", STREAMS, ids=IDS)
def test_parallel_equals_inflate_and_zlib(c):
    for S in spans():
        cap = len(c.want) if c.want is not None else 1000
        rc, n, _rep, buf, _ok = same_as_inflate(c, S, cap)
        if c.want is not None:
            assert (rc, n, buf) == (xb.OK, len(c.want), c.want)
        else:
            assert rc == xb.E_DATA


def test_parallel_equals_inflate_on_the_inflate_corpus():
    for c in icases.corpus():
        cap = wb.cap_for(c.stream, c.wrapper, c.want)
        for S in (256, xb.span_default()):
            got = same_as_inflate(c, S, cap)
            assert (got[0] == xb.OK) == (c.want is not None), c.name


def test_parallel_equals_inflate_on_the_table_mutations():
    for c in tc.mutated():
        for S in (256, xb.span_default()):
            got = same_as_inflate(c, S, tc.default_cap(c))
            assert (got[0] == xb.OK) == (c.want is not None), c.name


def test_parallel_equals_inflate_on_damaged_links():
    links = links_256()
    seen = set()
    for c in xc.mutated(links):
        rc, _n, rep, _buf, _ok = same_as_inflate(c, 256, 600000)
        assert (rc == xb.OK) == (c.want is not None), c.name
        same_as_inflate(c, 256, 1000)
        seen.add(rep["status"])
        if c.name.startswith("mutated/distance"):
            # the index cannot see it -- its table is whole -- and the tabled pass reports it first
            irc, n, _table, _chain, irep = xb.index(c.stream, 0, 256)
            assert (irc, irep["status"]) == (xb.OK, "OK") and n >= 3
            assert (rc, rep["status"], rep["out_pos"]) == (xb.E_DATA, "DISTANCE", 0 if "first" in c.name else 2)
    assert {"OK", "TRUNCATED", "DISTANCE"} <= seen and len(seen) >= 5, seen  # (a flip may leave a valid stream: zlib is the judge)


def test_short_buffers_around_every_seam_and_the_size_query():
    for name in ("zcut/phases", "oracle/pg11x3/fast/w0", "hand/phases", "zlib", "decoy/b"):
        c = by_name(name)
        _rc, _n, table, _chain, _rep = xb.index(c.stream, c.wrapper, 256)
        n = len(c.want)
        caps = {0, 1, n - 1, n, n + 1}
        for p in tc.starts([(t["bit_start"], t["in_bytes"]) for t in table]):
            caps |= {p - 1, p, p + 1}
        for cap in sorted(x for x in caps if 0 <= x <= n + 1):
            rc, got, _rep, buf, _ok = same_as_inflate(c, 256, cap, group=tc.GROUP_MIN)
            assert (rc, got) == (xb.OK if cap >= n else xb.E_OUT_TOO_SMALL, n) and buf[:min(cap, n)] == c.want[:cap]


def test_index_table_room():
    c = by_name("hand/phases")
    rc, n, _table, _chain, _rep = xb.index(c.stream, 0, 256)
    assert (rc, n) == (xb.OK, 9)
    assert xb.index(c.stream, 0, 256, cap=0)[:2] == (xb.E_OUT_TOO_SMALL, 9)  # the query
    assert xb.index(c.stream, 0, 256, cap=8)[:2] == (xb.E_OUT_TOO_SMALL, 9)
    assert xb.index(c.stream, 0, 256, cap=9)[:2] == (xb.OK, 9)
    c = by_name("hand/header_across_the_end")
    rc, n, table, _chain, rep = xb.index(c.stream, 0, 256)
    assert (rc, n) == (xb.E_DATA, 3) and sum(t["in_bytes"] for t in table) == rep["out_pos"] and rep["bit"] >= table[-1]["bit_start"]


# ---- mutants of the model: each is killed by a named case ----------------------------------------------------------------------------------
def differs_from_inflate(c, mutant):
    got = xb.parallel(c.stream, c.wrapper, 256, len(c.want), mutant=mutant)
    return got[:4] != wb.inflate(c.stream, c.wrapper, len(c.want))[:4]


def test_mutant_stop_at_or_beyond_the_candidate_is_killed_by_decoy_a():
    assert differs_from_inflate(by_name("decoy/a"), xb.MUTANT_STOP_GE)
    assert not differs_from_inflate(by_name("decoy/a"), 0)


def test_mutant_link_follows_the_candidate_is_killed_by_decoy_b():
    assert differs_from_inflate(by_name("decoy/b"), xb.MUTANT_LINK_CANDIDATE)
    assert differs_from_inflate(by_name("decoy/a"), xb.MUTANT_LINK_CANDIDATE)
    assert not differs_from_inflate(by_name("decoy/b"), 0)


def test_mutant_finder_accepts_bfinal_is_killed_by_hand_phases():
    c = by_name("hand/phases")
    true = set(true_starts(c))
    want = 1 + len({b // 2048 for b in true if b >= 2048})
    assert xb.index(c.stream, 0, 256)[1] == want
    assert xb.index(c.stream, 0, 256, mutant=xb.MUTANT_BFINAL)[1] == want + 1  # the BFINAL block begins in a span of its own
    assert xb.scan(c.stream, 0, 256, mutant=xb.MUTANT_BFINAL)[0] != xb.scan(c.stream, 0, 256)[0]
