"""The tabled inflate (deflate-rs_amd/csrc/inflate_table.h) as the host builds of tests/infltable run it over the cases of
inflate_table_cases.py: the three passes the kernels run -- symbols, windows, resolve, lane by lane and group by group -- give the
return value, the report and the buffer of the serial model on every case; a valid stream with a right table gives zlib's bytes and
the table-less report; a wrong table or a damaged stream never gives OK with bytes that are not zlib's; no symbol is loaded in front
of its fence; and the sanitizer program runs clean over all of it.  Every precondition of a case is asserted here, on the host build,
so that a case cannot silently stop forcing its edge.  CPU only."""
import os

import pytest

import inflate_table_cases as tc
import infltable_binding as tb


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: the passes have been run under ASan + UBSan, into exact-size buffers and workspaces, before anything else"""
    cases = [(c.stream, c.wrapper, c.table, c.gbytes, cap) for c, cap in tc.runs() if not tc.refused(c.table)]
    path = os.path.join(str(tmp_path), "corpus.bin")
    tb.write_corpus(path, cases)
    rc, out = tb.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


def by_name(name):
    return [c for c in tc.corpus() if c.name == name][0]


def run(c, cap=None, **kw):
    return tb.inflate(c.stream, c.wrapper, c.table, tc.default_cap(c) if cap is None else cap, group=c.gbytes, **kw)


def counted(c):
    tb.reset_counters()
    res = run(c)
    return res, tb.counters()


def test_preconditions_of_the_oracle_streams():
    c = by_name("oracle:pg11x3/default/w0")
    assert 170000 * 2 < len(c.want) < 600000 and len(c.table) >= 3
    assert any(bit % 8 for bit, _n in c.table)  # entries at bit offsets that are not byte aligned
    for level in ("fast", "default", "best", "rle"):
        (rc, _n, rep, _buf, _ok), cnt = counted(by_name("oracle:pg11x3/%s/w0" % level))
        assert rc == tb.OK and cnt["groups"] == 1
        if level != "rle":
            assert cnt["markers"] > 0, level  # matches reach back across entries
    (rc, _n, rep, _buf, _ok), cnt = counted(by_name("oracle:pg11x3/huffman_only/w0"))
    assert rc == tb.OK and cnt["markers"] == 0 and cnt["fences"] == 0
    (rc, _n, rep, _buf, _ok), cnt = counted(by_name("oracle:noise_200k/default/w0"))
    assert rc == tb.OK and rep["n_stored"] == rep["n_blocks"] > 1  # stored entries
    assert len(by_name("oracle:one_entry/default/w0").table) == 1
    # 64 KiB groups: the 500 KB input is several groups, every entry larger than the limit a group of its own
    c = by_name("oracle:pg11x3/default/w0/g64k")
    (rc, _n, _rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and cnt["groups"] == len(c.table) >= 3 and cnt["markers"] > 0


def test_preconditions_of_the_cut_streams():
    c = by_name("cut:lengths/w0")
    assert {n for _bit, n in c.table} >= {0, 1, 63, 64, 65, 32767, 32768, 32769, 40000}
    assert c.table[0][1] == 0 and all(bit % 8 == 0 for bit, _n in c.table)
    (rc, _n, _rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and cnt["markers"] > 0 and cnt["groups"] == 1
    g = by_name("cut:lengths/w0/g64k")
    (rc, _n, _rep, _buf, _ok), cnt = counted(g)
    assert rc == tb.OK and 2 <= cnt["groups"] < len(g.table) and cnt["markers"] > 0  # groups of several entries, windows across seams
    # every entry is copies of the one in front of it: a byte of the last one has come through every window
    c = by_name("cut:copies_of_copies/w0")
    assert len(c.table) == 8 and len(c.stream) < 25000
    (rc, _n, _rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and cnt["markers"] > 100000 and cnt["carry_depth"] >= 7, cnt
    (rc, _n, _rep, _buf, _ok), cnt = counted(by_name("cut:copies_of_copies/w0/g64k"))
    assert rc == tb.OK and cnt["groups"] >= 2 and cnt["carry_depth"] >= 7, cnt
    # the run crosses the cut
    c = by_name("cut:run_across_a_cut/w0")
    cutpos = c.table[0][1]
    assert c.want[cutpos - 1000:cutpos + 1000] == b"z" * 2000
    (rc, _n, _rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and cnt["markers"] > 0
    c = by_name("cut:stored_alignments/w0")
    assert {p % 8 for p in tc.starts(c.table)} == set(range(8)) and max(n for _b, n in c.table) > 65535
    (rc, _n, rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and rep["n_stored"] == rep["n_blocks"] and cnt["markers"] == 0
    # distance 32768 and distance 1 as the first token of an entry: both markers
    c = by_name("cut:first_byte_32768_and_1/w0")
    assert tc.starts(c.table) == [0, 32768, 32791]
    (rc, _n, _rep, _buf, _ok), cnt = counted(c)
    assert rc == tb.OK and cnt["markers"] == 20 + 258 + 70


def test_preconditions_of_the_wrong_tables_and_the_mutations():
    for base in ("z3", "o", "s3", "h3"):  # every kind of wrong table on every base: text, the oracle's, stored, Huffman only
        mine = [c for c in tc.wrong() if c.name.startswith("wrong:%s/" % base)]
        assert {c.name.split("/")[1].split("@")[0] for c in mine} == set(tc.WRONG_KINDS), base
        assert {c.name.split("/")[1] for c in mine} >= {"dropped@0", "dropped@1", "bit+1@1", "bit-1@1", "bytes+1@1", "bytes-1@1"}, base
        # refused from its numbers alone: the table without its first entry, and nothing else of these
        assert [c.name.split("/")[1] for c in mine if tc.refused(c.table)] == ["dropped@0"], base
    # nothing of a stored or a Huffman-only entry reaches in front of it: its data cannot give a wrong table away
    for base in ("s3", "h3"):
        c = by_name("wrong:%s/merged@1" % base)
        (rc, _n, _rep, _buf, _ok), cnt = counted(c)
        assert rc == tb.OK and cnt["markers"] == 0, base
    seen = set()
    for c in tc.mutated():
        seen.add(run(c)[2]["status"])
    assert seen >= {"OK", "FRAME", "TABLE", "TRUNCATED", "TRAILER", "CHECKSUM", "DISTANCE"}, seen
    per_entry = {k: sum(1 for c in tc.mutated() if c.name.endswith("@%d" % k)) for k in range(3)}
    assert min(per_entry.values()) >= 40
    assert any(c.caps for c in tc.oracle()) and any(c.caps for c in tc.cut())
    c = by_name("cut:lengths/w0")
    st = tc.starts(c.table)
    assert {0, 1, len(c.want) - 1, len(c.want), 20000, 40000, 40001} <= set(c.caps) and 40000 in st  # inside entry 0, on a seam, one beyond


@pytest.mark.parametrize("group", ["oracle", "cut", "wrong", "mutated"])
def test_the_three_passes_equal_the_serial_model(group):
    n = 0
    for c, cap in tc.runs():
        if c.group != group:
            continue
        n += 1
        serial = run(c, cap, three=False)
        three = run(c, cap, three=True)
        assert three == serial, (c.name, cap, serial[:3], three[:3])
        rc, got, rep, buf, canary = three
        if tc.refused(c.table):  # MI355_E_ARG, and nothing written
            assert (rc, got, buf) == (tb.E_ARG, 0, b"\xA5" * cap) and canary, c.name
            continue
        assert canary, (c.name, cap)
        assert rep["status"] in tb.TABLED_STATUS, (c.name, rep)
        if group in ("oracle", "cut"):
            size = len(c.want)
            assert (rc, got, rep["status"], rep["out_len"]) == (tb.OK if cap >= size else tb.E_OUT_TOO_SMALL, size, "OK", size), (c.name, cap, rep)
            assert buf == c.want[:cap], (c.name, cap)
            # blocks=None: the same bytes, and the same report -- the block counts of a tabled call are the sums over the entries
            assert tb.inflate(c.stream, c.wrapper, None, cap) == three, (c.name, cap)
            continue
        if rc == tb.OK:  # never OK with bytes that are not zlib's
            assert c.want is not None and buf == c.want and got == len(c.want), c.name
        else:
            assert rc == tb.E_DATA and rep["status"] != "OK", (c.name, rep)
            assert got == min(rep["out_pos"], cap) and rep["out_len"] == 0, (c.name, rep)
            assert buf[got:] == b"\xA5" * (cap - got), c.name  # nothing written at or beyond out_pos
            if c.want is not None and group == "mutated":  # (the table is right: the entries in front of the failure are the serial walk)
                assert buf[:got] == c.want[:got], c.name  # ... and in front of it, the stream's bytes
        if group == "wrong" and "/merged@" not in c.name:
            assert rc == tb.E_DATA, (c.name, rep)
    assert n > 30
    assert tb.counters()["unfenced"] == 0


def test_a_wrong_table_is_table_where_the_entries_do_not_meet():
    for name in ("bit+1@1", "bit-1@1", "bytes+1@1", "bytes-1@1", "total+1", "total-1", "bfinal_not_last"):
        c = by_name("wrong:z3/" + name)
        rc, _got, rep, _buf, _ok = run(c)
        assert (rc, rep["status"]) == (tb.E_DATA, "TABLE"), (name, rep)
    for name in ("merged@1", "merged@2"):  # a coarser table that is right
        c = by_name("wrong:z3/" + name)
        rc, got, rep, buf, _ok = run(c)
        assert (rc, rep["status"], buf) == (tb.OK, "OK", c.want), (name, rep)


def test_the_trailer_is_judged_over_the_output():
    assert run(by_name("mutated:zlib_adler"))[2]["status"] == "CHECKSUM"
    assert run(by_name("mutated:gzip_crc"))[2]["status"] == "CHECKSUM"
    assert run(by_name("mutated:gzip_isize"))[2]["status"] == "CHECKSUM"
    assert run(by_name("mutated:zlib_byte_behind"))[2]["status"] == "TRAILER"
    assert run(by_name("mutated:gzip_header"))[2]["status"] == "FRAME"
    # a checksum is not judged when the buffer is short
    c = by_name("mutated:zlib_adler")
    n = tc.total(c.table)
    rc, got, rep, _buf, _ok = run(c, n - 1)
    assert (rc, got, rep["status"]) == (tb.E_OUT_TOO_SMALL, n, "OK")


def test_argument_errors():
    import ctypes as C
    L = tb.lib()
    r, n = tb.Report(), C.c_uint64(0)
    two = (C.c_uint64 * 2)
    s = b"\x03\x00"
    assert L.infltable_inflate(1, s, 2, 0, two(8, 0), two(0, 0), 2, tb.GROUP_DEFAULT, None, 0, C.byref(n), C.byref(r)) == tb.E_ARG  # bits descend
    assert L.infltable_inflate(1, s, 2, 0, two(8, 16), two(0, 0), 2, tb.GROUP_DEFAULT, None, 0, C.byref(n), C.byref(r)) == tb.E_ARG  # not from bit 0
    assert L.infltable_inflate(0, s, 2, 0, two(1, 0), two(0, 0), 1, tb.GROUP_DEFAULT, None, 0, C.byref(n), C.byref(r)) == tb.E_ARG
    assert L.infltable_inflate(1, s, 2, 3, two(0, 0), two(0, 0), 1, tb.GROUP_DEFAULT, None, 0, C.byref(n), C.byref(r)) == tb.E_ARG
    assert L.infltable_inflate(1, s, 2, 0, two(0, 0), two(0, 0), 1, tb.GROUP_DEFAULT, None, 5, C.byref(n), C.byref(r)) == tb.E_ARG
    assert L.infltable_inflate(1, s, 2, 0, two(0, 0), two(0, 0), 1, tb.GROUP_MIN - 1, None, 0, C.byref(n), C.byref(r)) == tb.E_ARG
    assert L.infltable_inflate(1, s, 2, 0, two(0, 0), two(0, 0), 1, tb.GROUP_MIN, None, 0, C.byref(n), C.byref(r)) == tb.OK and n.value == 0
    assert L.infltable_inflate(1, s, 2, 0, None, None, 0, tb.GROUP_MIN, None, 0, C.byref(n), C.byref(r)) == tb.OK  # no table
