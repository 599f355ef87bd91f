"""The model of the BGZF encode (bgzf_cases.py) judged without a GPU: every model file is read by Python's gzip, every BSIZE is true,
the marker is last, no member is longer than BSIZE can say, the .gzi index agrees with the offsets, the case set covers the residues
and seams the gather kernel can go wrong at -- and three mutants of the model are each caught by the same checks.  CPU only."""
import os
import struct
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "deflate-rs_amd"))

import bgzf_cases as bc

CASES = bc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_files_are_bgzf(case):
    file, members = bc.model(case.data, case.level, case.block)
    bc.check_file(file, members, case.data, case.block)
    assert members[-1]["out_len"] == 0 and members[-1]["in_len"] == 28 and file.endswith(bc.EOF)
    assert sum(m["in_len"] for m in members) == len(file)


def test_the_marker_is_the_oracles_member_of_the_empty_input():
    import oracle_binding as ob
    for lv, (preset, _o) in bc.LEVELS.items():
        assert bc.patch(ob.encode_gzip(b"", bc.H, level=preset)) == bc.EOF, lv
    file, members = bc.model(b"", "default", 0)
    assert file == bc.EOF and len(members) == 1


def test_one_byte_gives_a_member_of_29_bytes_and_a_file_of_57():
    file, members = bc.model(b"x", "default", 0)
    assert [m["in_len"] for m in members] == [29, 28] and len(file) == 57


def test_the_small_block_case_runs_more_than_one_round_of_the_scan():
    (c,) = bc.small()
    _file, members = bc.model(c.data, c.level, c.block)
    assert len(members) == 1563 + 1 > 1024
    lens = [m["in_len"] for m in members[:-1]]
    assert 29 <= min(lens) and max(lens) <= 18 + 5 + 64 + 8  # (a stored slice at the most)


def test_members_always_fit_bsize():
    """noise is the longest a member gets: 26 bytes of frame and three stored blocks of 5 bytes around the bytes themselves"""
    longest = 0
    for c in bc.noise():
        _file, members = bc.model(c.data, c.level, c.block)
        longest = max(longest, max(m["in_len"] for m in members))
    assert longest == bc.BLOCK_MAX + 41 <= bc.MEMBER_MAX
    for c in CASES:
        assert all(m["in_len"] <= bc.MEMBER_MAX for m in bc.model(c.data, c.level, c.block)[1])


def test_gzi_agrees_with_the_offsets():
    import deflate_amd as da
    for c in CASES:
        file, members = bc.model(c.data, c.level, c.block)
        idx = da.bgzf_gzi(members)
        assert idx == bc.gzi(members) == da.bgzf_gzi(members[:-1])
        (n,) = struct.unpack_from("<Q", idx)
        assert n == max(len(members) - 2, 0) and len(idx) == 8 + 16 * n
        b = c.block or bc.BLOCK_MAX
        for k in range(n):
            coff, uoff = struct.unpack_from("<QQ", idx, 8 + 16 * k)
            assert uoff == (k + 1) * b and file[coff: coff + 16] == bc.H[:16] and coff == members[k + 1]["in_off"]


def test_the_cases_cover_the_gathers_residues_and_seams():
    starts, lens, seams = bc.coverage()
    assert starts == set(range(16))
    assert lens == set(range(16))
    assert seams == set(range(1, 16))
    s1, l1, _ = bc.coverage(bc.small())  # (that case alone has every start and every length)
    assert s1 == set(range(16)) and l1 == set(range(16))


def _mutants(case):
    parts = list(bc.model_parts(case.data, case.level, case.block))
    lens = [len(s) for s in bc.slices(case.data, case.block)]
    off = parts[1][:16] + struct.pack("<H", len(parts[1])) + parts[1][18:]  # BSIZE one too many
    yield "bsize", parts[:1] + [off] + parts[2:], lens
    yield "pad", parts[:1] + [parts[1] + b"\0"] + parts[2:], lens  # (Python's gzip skips zero padding: the walk does not)
    yield "swap", [parts[1], parts[0]] + parts[2:], [lens[1], lens[0]] + lens[2:]


def test_mutants_of_the_model_are_caught():
    (case,) = [c for c in CASES if c.name == "three-default"]
    file, members = bc.model(case.data, case.level, case.block)
    bc.check_file(file, members, case.data, case.block)
    for name, parts, lens in _mutants(case):
        bad = b"".join(parts)
        assert bad != file
        with pytest.raises(AssertionError):
            bc.check_file(bad, bc.rows_of(parts, lens), case.data, case.block)
