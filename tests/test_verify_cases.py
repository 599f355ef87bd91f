"""The verify decisions (deflate-rs_amd/csrc/inflate_check.h) as the host build of tests/inflcheck runs them, over the cases of
verify_cases.py: valid streams verify, with and without the oracle's block table; for mutated and hand-assembled streams the
verdict is zlib's, in both directions; an edited input is found at the edited byte; and the sanitizer program runs clean over all
of it.  CPU only."""
import os

import pytest

import inflcheck_binding as ib
import verify_cases as vc


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: nothing of the corpus goes anywhere before the decoder has been run over it under ASan + UBSan"""
    path = os.path.join(str(tmp_path), "corpus.bin")
    cases = list(vc.corpus())
    ib.write_corpus(path, cases)
    rc, out = ib.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


def test_valid_streams_verify_without_a_table():
    for name, stream, data, wrapper, _tab in vc.streams():
        rc, rep = ib.verify(stream, data, wrapper)
        assert (rc, rep["status"]) == (ib.OK, "OK"), (name, rep)
        assert rep["n_blocks"] == rep["n_stored"] + rep["n_fixed"] + rep["n_dynamic"] >= 1, (name, rep)


def test_oracle_streams_verify_with_the_oracles_table():
    seen = 0
    for name, stream, data, wrapper, tab in vc.streams():
        if not tab:
            continue
        table, trace = tab
        rc, rep = ib.verify(stream, data, wrapper, table)
        assert (rc, rep["status"]) == (ib.OK, "OK"), (name, rep)
        # a stored block of the encoder is a run of pieces of at most 32767 bytes (one, empty, for no bytes)
        pieces = sum(max(1, -(-n // 32767)) for (_, n), t in zip(table, trace) if t == 0)
        assert (rep["n_stored"], rep["n_fixed"], rep["n_dynamic"]) == (pieces, trace.count(1), trace.count(2)), (name, rep, trace)
        assert rep["n_blocks"] == pieces + trace.count(1) + trace.count(2)
        seen += len(table) > 1
    assert seen >= 10  # tables of several entries among them


def test_table_errors():
    name, stream, data, wrapper, tab = next(c for c in vc.streams() if c[4] and len(c[4][0]) >= 5)
    table = list(tab[0])
    bad = list(table)
    bad[3] = (bad[3][0] + 1, bad[3][1])
    rc, rep = ib.verify(stream, data, wrapper, bad)
    assert rc == ib.E_VERIFY and rep["status"] == "TABLE" and rep["entry"] in (2, 3), rep
    rc, _ = ib.verify(stream, data, wrapper, [table[1], table[0]] + table[2:])
    assert rc == ib.E_ARG
    rc, _ = ib.verify(stream, data, wrapper, table[:-1])
    assert rc == ib.E_ARG


@pytest.mark.parametrize("group", ["mutations", "hand"])
def test_verdict_is_zlibs(group):
    """twin OK <=> zlib inflates the stream to exactly the input, reaches its end and leaves nothing over; no case left out"""
    cases = vc.mutations() if group == "mutations" else vc.hand()
    ok = 0
    for c in cases:
        name, stream, data, wrapper = c[:4]
        rc, rep = ib.verify(stream, data, wrapper)
        want = vc.zlib_accepts(stream, data, wrapper)
        assert (rc == ib.OK) == want and (rep["status"] == "OK") == want, (name, rep, want)
        ok += want
    assert 0 < ok < len(cases)
    if group == "mutations":  # pad bits were among the flipped ones: such a flip leaves the stream valid
        assert any(c[0].endswith("p") and vc.zlib_accepts(c[1], c[2], c[3]) for c in cases if c[0].startswith("raw/"))
        assert any(c[0].endswith("p") and vc.zlib_accepts(c[1], c[2], c[3]) for c in cases if c[0].startswith("zlib/"))


def test_hand_assembled_streams_give_their_status():
    for name, stream, data, wrapper, status in vc.hand():
        rc, rep = ib.verify(stream, data, wrapper)
        assert rep["status"] == status, (name, rep)
        assert rc == (ib.OK if status == "OK" else ib.E_VERIFY)


def test_framed_failures_have_their_status():
    by = {c[0]: c for c in vc.mutations()}
    for name, status in (("zlib/append1", "TRAILER"), ("raw/append4", "TRAILER"), ("zlib/trailer1", "CHECKSUM"), ("zlib/trailer4", "CHECKSUM"),
                         ("raw/trunc1", "TRUNCATED")):
        _, stream, data, wrapper = by[name]
        assert ib.verify(stream, data, wrapper)[1]["status"] == status, name
    data = vc.pg11()[:20000]
    gz = next(c for c in vc.streams() if c[0] == "pg11_20000/o1/gzip_all")
    for k, status in ((0, "FRAME"), (2, "FRAME"), (3, "FRAME"), (len(gz[1]) - 8, "CHECKSUM"), (len(gz[1]) - 1, "CHECKSUM")):
        m = bytearray(gz[1])
        m[k] ^= 0x80
        assert ib.verify(bytes(m), data, 2)[1]["status"] == status, k
    assert ib.verify(gz[1][:17], data, 2)[1]["status"] == "FRAME"
    assert ib.verify(b"\x78\x9c\x03\x00\x00", b"", 1)[1]["status"] == "FRAME"  # shorter than header + trailer


def test_input_edits_are_found_at_the_edited_byte():
    for name, stream, data, wrapper, k in vc.edits():
        rc, rep = ib.verify(stream, data, wrapper)
        assert (rc, rep["status"], rep["in_pos"]) == (ib.E_VERIFY, "MISMATCH", k), (name, rep)


def test_lds_fits_eight_workgroups_a_cu_many_times():
    assert ib.lib().inflcheck_tables_size() <= 160 * 1024 // 8
