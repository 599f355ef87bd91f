"""The inflate decisions (deflate-rs_amd/csrc/inflate_write.h) as the host build of tests/inflwrite runs them, scalar and lane by
lane, over the cases of inflate_cases.py: what zlib accepts inflates to zlib's bytes, what it refuses is MI355_E_DATA, a short
buffer gets the exact size and its prefix and nothing behind it, and the sanitizer program runs clean over all of it.  CPU only."""
import os

import pytest

import inflate_cases as icase
import inflwrite_binding as iw


def test_sanitizer_program_runs_clean_over_the_corpus(tmp_path):
    """first in the file: the decoder has been run under ASan + UBSan, into exact-size buffers, before anything else uses it"""
    cases = []
    for c in icase.corpus():
        if c.want is None:
            cases.append((c.stream, c.wrapper, 20000))  # (the mutations' input is 20 000 bytes: some stop short, some run past)
            continue
        cases.append((c.stream, c.wrapper, len(c.want)))
        if c.group in ("hand", "write_path", "framed") or len(c.want) < 4096:
            cases += [(c.stream, c.wrapper, cap) for cap in (0, 1, len(c.want) - 1, len(c.want) // 2) if 0 <= cap < len(c.want)]
    path = os.path.join(str(tmp_path), "corpus.bin")
    iw.write_corpus(path, cases)
    rc, out = iw.run_fuzz(path)
    assert rc == 0, out
    assert out.startswith("%d cases:" % len(cases)), out


def test_preconditions_of_the_corpus():
    for c in icase.corpus():
        if c.group == "write_path":
            assert c.want is not None, c.name  # every hand-assembled write-path case is a valid stream
    assert len(icase.accepted()) >= 50
    seen = set()
    for c in icase.rejected():
        rc, n, rep, _buf, _ok = iw.inflate(c.stream, c.wrapper, iw.cap_for(c.stream, c.wrapper, None))
        assert rc == iw.E_DATA, (c.name, rep)
        seen.add(rep["status"])
    assert seen >= {"FRAME", "BTYPE", "STORED", "LENGTHS", "CODE", "DISTANCE", "TRUNCATED", "TRAILER", "CHECKSUM"}, seen
    # hand()'s streams that only fail against their input are valid streams for an inflater
    by_name = {c.name: c for c in icase.corpus()}
    for name in ("token_past_in_len", "bfinal_before_in_len", "literal_differs"):
        assert by_name["hand:" + name].want is not None


@pytest.mark.parametrize("group", ["streams", "mutations", "hand", "write_path", "framed"])
def test_verdict_and_bytes_are_zlibs(group):
    """accepted <=> MI355_OK with zlib's bytes; rejected <=> MI355_E_DATA; scalar and lane by lane the same report and bytes"""
    fences0 = iw.lib().inflwrite_fences()
    n = 0
    for c in icase.corpus():
        if c.group != group:
            continue
        n += 1
        cap = iw.cap_for(c.stream, c.wrapper, c.want)
        rc, got, rep, buf, canary = iw.inflate(c.stream, c.wrapper, cap)
        rc2, got2, rep2, buf2, canary2 = iw.inflate(c.stream, c.wrapper, cap, lanes=True)
        assert (rc, got, rep, buf) == (rc2, got2, rep2, buf2), (c.name, rep, rep2)
        assert canary and canary2, c.name
        assert rep["status"] in iw.INFLATE_STATUS, (c.name, rep)
        if c.want is not None:
            assert (rc, rep["status"], got) == (iw.OK, "OK", len(c.want)), (c.name, rep)
            assert buf == c.want, c.name
            assert rep["out_pos"] == rep["out_len"] == len(c.want) and rep["bit"] == 0, (c.name, rep)
            assert rep["n_blocks"] == rep["n_stored"] + rep["n_fixed"] + rep["n_dynamic"] >= 1, (c.name, rep)
        else:
            assert rc == iw.E_DATA and rep["status"] != "OK", (c.name, rep)
            assert got == min(rep["out_pos"], cap) and rep["out_len"] == 0, (c.name, rep)
            assert buf[got:] == b"\xA5" * (cap - got), c.name  # nothing written at or beyond out_pos
        if c.label in iw.INFLATE_STATUS:
            assert rep["status"] == c.label, (c.name, rep)
    assert n > 0
    assert iw.lib().inflwrite_unfenced_loads() == 0
    if group == "write_path":  # the overlapping matches did need their fences
        assert iw.lib().inflwrite_fences() > fences0


def test_a_failure_leaves_the_bytes_in_front_of_it():
    """truncations of a valid stream: out[0, out_pos) is the prefix of what the whole stream inflates to"""
    base, data, wrapper, _ = __import__("verify_cases").mutation_base()[0]
    for cut in (1, 2, 3, 100, 1000, len(base) // 2):
        rc, got, rep, buf, canary = iw.inflate(base[:-cut], wrapper, len(data), lanes=True)
        assert rc == iw.E_DATA and rep["status"] == "TRUNCATED" and canary, rep
        assert got == rep["out_pos"] and buf[:got] == data[:got], (cut, rep)


def test_short_buffers_get_the_size_the_prefix_and_nothing_behind_it():
    checked = 0
    for c in icase.accepted():
        n = len(c.want)
        lanes = c.group in ("hand", "write_path", "framed")
        for cap in sorted({0, 1, n - 1, n}):
            if not 0 <= cap <= n:
                continue
            rc, got, rep, buf, canary = iw.inflate(c.stream, c.wrapper, cap, lanes=lanes)
            assert canary, (c.name, cap)
            assert (rc, got, rep["out_len"]) == (iw.OK if cap >= n else iw.E_OUT_TOO_SMALL, n, n), (c.name, cap, rep)
            assert rep["status"] == "OK" and buf == c.want[:cap], (c.name, cap)
            checked += 1
    assert checked >= 200


def test_a_checksum_is_not_judged_when_the_buffer_is_short():
    by_name = {c.name: c for c in icase.corpus()}
    c, good = by_name["framed:zlib_adler_low"], by_name["framed:zlib_ok"]
    n = len(good.want)
    assert iw.inflate(c.stream, 1, n)[2]["status"] == "CHECKSUM"
    rc, got, rep, buf, _ = iw.inflate(c.stream, 1, n - 1)
    assert (rc, got, rep["status"]) == (iw.E_OUT_TOO_SMALL, n, "OK") and buf == good.want[:n - 1]
    # ... while a structural failure is reported whatever the buffer holds
    t = by_name["framed:zlib_byte_behind"]
    assert iw.inflate(t.stream, 1, 0)[0] == iw.E_DATA and iw.inflate(t.stream, 1, 0)[2]["status"] == "TRAILER"


def test_argument_errors():
    L = iw.lib()
    r = iw.Report()
    import ctypes as C
    n = C.c_uint64(0)
    assert L.inflwrite_inflate(b"\x03\x00", 2, 3, None, 0, C.byref(n), C.byref(r)) == iw.E_ARG
    assert L.inflwrite_inflate(b"\x03\x00", 2, 0, None, 5, C.byref(n), C.byref(r)) == iw.E_ARG
    assert L.inflwrite_inflate(b"\x03\x00", 2, 0, None, 0, C.byref(n), C.byref(r)) == iw.OK and n.value == 0
