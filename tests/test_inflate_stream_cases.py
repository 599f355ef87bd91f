"""The streaming inflate decisions on the host (tests/inflstream: inflate_stream.h with a scalar and a lane-by-lane sink, and a model of
the handle): every case of inflate_stream_cases through both sinks against zlib and the one-shot host build, the sanitizer program
over the corpus, and five mutants of the model, each caught by a named case."""
import os

import pytest

import inflate_stream_cases as isc
import inflstream_binding as sb


def _run_all(lanes, only=None):
    for s in isc.scripts():
        if only and not s.name.startswith(only):
            continue
        h = sb.Model(s.wrapper, s.zdict, lanes=lanes)
        try:
            isc.judge(s, isc.run(h, s))
        finally:
            h.close()


def test_cells_are_covered():
    assert set(isc.CELLS) <= isc.coverage()
    kinds = {s.kind for s in isc.scripts()}
    assert kinds == {"valid", "prefix", "fail", "explicit", "reset"}
    assert sum(1 for s in isc.scripts() if s.kind == "fail" and s.name.startswith("fail")) > 300


@pytest.mark.parametrize("lanes", [False, True], ids=["scalar", "lanes"])
def test_every_case_against_zlib_and_the_one_shot(lanes):
    sb.set_mutant(None)
    before = sb.lib().ism_unfenced_loads()
    _run_all(lanes)
    assert sb.lib().ism_unfenced_loads() == before, "a lane loaded output bytes that no fence had made loadable"


def test_frame_prefix_agrees_with_the_whole_header():
    for _tag, s, w, _d in isc.bases():
        n = isc.hdr_len(w)
        for k in range(0, n):
            assert sb.frame_prefix(s[:k], w) == (sb.FP_NEED_MORE, 0), (w, k)
        for k in (n, n + 1, len(s)):
            assert sb.frame_prefix(s[:k], w) == (sb.FP_OK, n), (w, k)
    assert sb.frame_prefix(b"\x78\xbb", 1)[0] == sb.FP_BAD       # FDICT
    assert sb.frame_prefix(b"\x77", 1)[0] == sb.FP_BAD            # CM 7, with one byte
    assert sb.frame_prefix(b"\x1f\x8c", 2)[0] == sb.FP_BAD
    assert sb.frame_prefix(b"\x1f\x8b\x08\x80", 2)[0] == sb.FP_BAD  # a reserved flag
    long_name = b"\x1f\x8b\x08\x08" + bytes(6) + b"x" * (65536 + 32)
    assert sb.frame_prefix(long_name[:5000], 2)[0] == sb.FP_NEED_MORE
    assert sb.frame_prefix(long_name, 2)[0] == sb.FP_BAD           # no end inside 64 KiB + 32


def test_sanitizer_program_over_the_corpus(tmp_path):
    path = os.path.join(str(tmp_path), "corpus.bin")
    sb.write_corpus(path, isc.fuzz_corpus())
    rc, out = sb.run_fuzz(path)
    assert rc == 0, out


# a mutant of the model and the case that catches it
MUTANTS = [
    ("history_not_shifted", "update:1"),
    ("seam_off_by_one", "hist:dist_1"),
    ("commit_inside_block", "split2:raw@100"),
    ("truncated_is_final", "split2:zlib@200"),
    ("dist_this_write_only", "hist:dist_hist_len"),
]


@pytest.mark.parametrize("mutant,case", MUTANTS, ids=[m for m, _ in MUTANTS])
@pytest.mark.parametrize("lanes", [False, True], ids=["scalar", "lanes"])
def test_mutant_is_caught(mutant, case, lanes):
    s, = [x for x in isc.scripts() if x.name == case]
    try:
        sb.set_mutant(mutant)
        h = sb.Model(s.wrapper, s.zdict, lanes=lanes)
        with pytest.raises(AssertionError):
            isc.judge(s, isc.run(h, s))
        h.close()
    finally:
        sb.set_mutant(None)
    h = sb.Model(s.wrapper, s.zdict, lanes=lanes)
    isc.judge(s, isc.run(h, s))
    h.close()
