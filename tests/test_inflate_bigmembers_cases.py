"""The large plain members of the members inflate (deflate-rs_amd/csrc/inflate_bigmembers.h) as the host build of tests/inflbig runs
them over the cases of inflate_bigmembers_cases.py.  On every case, at both index spans, with groups of 64 KiB and of the default size
and at every short buffer, the call with the parallel path on equals the serial model of tests/inflmembers -- return value, length,
every report field, the whole member table with its flags, the bytes that hold data, the canary behind out_cap -- and, through it,
the plain serial walk and zlib.  On a valid file the number of members the parallel path decoded is the case's expected number: a
valid member never falls back.  The index spans searched stay proportional to the file.  Every mutant of the new decisions is
caught.  CPU only."""
import os

import pytest

import inflate_bigmembers_cases as bc
import inflbig_binding as bb
import inflmembers_binding as mb

CASES = bc.corpus()
IDS = [c.name for c in CASES]
T = bc.THRESHOLD
MEMBER_SPAN = 65536
SETTINGS = [(bc.SPANS[0], bc.GROUP_SMALL), (bc.SPANS[1], bb.GROUP_DEFAULT)]  # (index span, group bytes)


def own_cap(c):
    if c.want is not None:
        return len(c.want)
    rc, n, _rep, _m, _d, _ok = mb.serial(c.stream, 0)
    return n if rc == mb.E_OUT_TOO_SMALL else 70000


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: discovery and the three passes have run under ASan + UBSan, with exact-size file, output, table, candidate,
    symbol and window allocations, before anything else"""
    cases = []
    for c in CASES:
        for S, g in SETTINGS:
            cases.append((c.stream, own_cap(c), MEMBER_SPAN, T, S, g))
        for cap in c.caps:
            cases.append((c.stream, cap, MEMBER_SPAN, T, bc.SPANS[0], bc.GROUP_SMALL))
    path = os.path.join(str(tmp_path), "corpus.bin")
    bb.write_corpus(path, cases)
    rc, out = bb.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_serial_walk_agrees_with_zlib(c):
    rc, n, rep, members, data, ok = mb.serial(c.stream, own_cap(c))
    assert ok
    if c.want is not None:
        assert (rc, n, data, rep["status"]) == (mb.OK, len(c.want), c.want, "OK"), rep
        assert sum(m[1] for m in members) == len(c.stream) and all(m[5] == "OK" for m in members)
    else:
        assert rc == mb.E_DATA and rep["status"] != "OK" and members[-1][5] == rep["status"], rep
        assert len(members) == c.facts["damaged"] + 1


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_call_equals_the_serial_model(c):
    for cap in (own_cap(c),) + c.caps:
        model = mb.run(c.stream, MEMBER_SPAN, cap)
        assert model[5] and mb.structure(model) == mb.structure(mb.serial(c.stream, cap))
        for S, g in SETTINGS:
            got, st = bb.run(c.stream, MEMBER_SPAN, cap, T, S, g)
            assert got == model, (c.name, S, g, cap, got[:4], model[:4])
            if c.expect is not None:
                # a condition, not a measurement: a walker links only on a candidate at a true block boundary
                assert (st["parallel"], st["handed"]) == (c.expect, sum(1 for m in model[3] if not m[4]) - c.expect), (c.name, S, cap, st)
            elif model[2]["status"] == "CHECKSUM":
                assert st["parallel"] == 3, (c.name, S, st)  # structurally clean: the checksum pass judges the member table afterwards
            else:
                assert st["parallel"] <= c.facts["damaged"], (c.name, S, st)  # nothing behind the damage is reported from this path
            # the extent rule: the spans searched are proportional to the file, not members x file
            members = len(model[3])
            assert st["spans"] <= 2 * (len(c.stream) / S) + members * bb.first_extent(T, S) + members, (c.name, S, st)
            assert st["walkers"] >= st["spans"] or not st["spans"]


@pytest.mark.parametrize("c", [c for c in CASES if c.want is not None], ids=[c.name for c in CASES if c.want is not None])
def test_switched_off_it_is_the_serial_model_and_counts_nothing(c):
    got, st = bb.run(c.stream, MEMBER_SPAN, own_cap(c), 0, bc.SPANS[0], bc.GROUP_SMALL)
    assert got == mb.run(c.stream, MEMBER_SPAN, own_cap(c)) and not any(st.values())
    assert got[4] == c.want


def test_short_buffers_and_the_size_query():
    c = bc.by_name("short/plain3")
    assert 0 in c.caps and len(c.caps) >= 12
    for cap in c.caps:
        (rc, n, rep, members, data, ok), st = bb.run(c.stream, MEMBER_SPAN, cap, T, bc.SPANS[0], bc.GROUP_SMALL)
        assert ok and data == c.want[:cap] and st["parallel"] == 3
        assert (rc, n) == (mb.OK if cap >= len(c.want) else mb.E_OUT_TOO_SMALL, len(c.want)), cap
        assert len(members) == 3 and rep["out_len"] == len(c.want)


# ---- preconditions of the named cases -----------------------------------------------------------------------------------------------
def stats(name, S, g=bb.GROUP_DEFAULT):
    c = bc.by_name(name)
    return bb.run(c.stream, MEMBER_SPAN, len(c.want), T, S, g)[1]


def test_groups_hold_parts_of_members_and_members_span_groups():
    st = stats("valid/three_groups", bc.SPANS[0], bc.GROUP_SMALL)
    assert st["sets"] >= 4  # the first member alone is 260 000 bytes: three groups of 64 KiB at least, and one for the member behind it
    st = stats("valid/group_of_three", bc.SPANS[0], bc.GROUP_SMALL)
    assert (st["parallel"], st["sets"]) == (3, 1) and st["entries"] >= 3  # 60 000 bytes: one group, parts of three members


def test_a_boundary_at_the_edge_makes_the_extent_grow():
    """the member in the middle on its own: where the BFINAL block ends at the edge, or a bit behind it, the first extent is all it
    searches; where another block follows the boundary there, the extent grows"""
    for S in bc.SPANS:
        def lone(kind):
            c = bc.by_name("valid/edge/%d/%s" % (S, kind))
            m = c.stream[c.facts["starts"][1]: c.facts["starts"][2]]
            got, st = bb.run(m, MEMBER_SPAN, 70000, T, S, bb.GROUP_DEFAULT)
            assert got[0] == mb.OK and st["parallel"] == 1
            return st["spans"]
        assert lone("final0") == lone("final1") == bb.first_extent(T, S)
        assert lone("boundary0") > bb.first_extent(T, S) and lone("boundary1") > bb.first_extent(T, S)


def test_a_hinted_header_behind_a_member_costs_no_round():
    """the chain stops at the BGZF run behind the plain member on the member's head alone: the spans searched are the plain member's"""
    c = bc.by_name("valid/bgzf_plain_bgzf")
    st0 = c.facts["starts"]
    lone = c.stream[st0[4]: st0[5]]
    for S in bc.SPANS:
        alone = bb.run(lone, MEMBER_SPAN, 70000, T, S, bb.GROUP_DEFAULT)[1]
        whole = bb.run(c.stream, MEMBER_SPAN, len(c.want), T, S, bb.GROUP_DEFAULT)[1]
        assert alone["parallel"] == whole["parallel"] == 1 and (whole["spans"], whole["walkers"]) == (alone["spans"], alone["walkers"])


def test_one_entry_members_go_into_the_joint_launch():
    for name in ("valid/stored_only", "valid/one_fixed_block"):
        c = bc.by_name(name)
        lone = c.stream[c.facts["starts"][1]: c.facts["starts"][2]]
        got, st = bb.run(lone, MEMBER_SPAN, len(c.want), T, bc.SPANS[0], bc.GROUP_SMALL)
        assert got[0] == mb.OK and (st["parallel"], st["entries"], st["sets"]) == (1, 1, 1), (name, st)


# ---- the mutants --------------------------------------------------------------------------------------------------------------------
def killers(mutant):
    out = []
    for c in CASES:
        got, _st = bb.run(c.stream, MEMBER_SPAN, own_cap(c), T, bc.SPANS[0], bc.GROUP_SMALL, mutant=mutant)
        if got != mb.run(c.stream, MEMBER_SPAN, own_cap(c)):
            out.append(c.name)
    return out


def test_a_distance_limited_by_the_files_position_is_caught():
    """the member in front lies right there: the mutant takes its bytes for history and reports no DISTANCE"""
    k = killers(bb.MUTANT_FILE_POSITION)
    assert "damage/middle/far_distance" in k and "damage/last/far_distance" in k, k
    assert not [n for n in k if n.startswith("valid/")], k  # (a valid file never looks in front of its member)


def test_a_trailer_one_byte_off_behind_a_byte_boundary_is_caught():
    k = killers(bb.MUTANT_TRAILER_OFF)
    assert "valid/ends_on_a_byte" in k and "valid/ends_inside_a_byte" not in k, k
