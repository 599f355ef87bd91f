"""Streams written in pieces and flushed, on the GPU: the cases of tests/flush_cases.py through DeflateEncoder / ZlibEncoder /
GzEncoder, bit-exact against the oracle.  Every case puts a flush point, a position the write pattern files differently, or the end
of the kept history on the geometry of a kernel that reads it (tests/test_flush_cases.py asserts on the CPU that each case does, on
the oracle alone).  After every flush the bytes handed out so far must be the oracle's, so a failure names the flush that went
wrong, and flush_cases.flush_diff names the first differing token, its position and epoch, and the lists the model derives for that
call.  pytest -m gpu."""
import io
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import flush_cases as fc
import oracle_binding as ob

pytestmark = pytest.mark.gpu

MI355_FLUSH_SYNC = 1  # include/mi355_deflate.h


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


def run_case(da, ctx, c, wrapper=0):
    """the case's script through the encoder of that wrapper; every flush and the finished stream against the oracle"""
    cls = (da.DeflateEncoder, da.ZlibEncoder, da.GzEncoder)[wrapper]
    if wrapper == 0:
        ref, marks, sums = fc.oracle(c)
    else:
        ref, marks, sums = fc.run_oracle(c["data"], c["opts"], c["script"], wrapper, da.BLANK_GZIP_HEADER if wrapper == 2 else None)
    sink = io.BytesIO()
    enc = cls(sink, da.CompressionOptions(*c["opts"]), ctx)
    data, p, k = c["data"], 0, 0
    for op in c["script"]:
        if op != "F":
            enc.write_all(data[p:p + op])
            p += op
            continue
        enc.flush()
        got = sink.getvalue()
        if got != ref[:marks[k]]:
            skip = {0: 0, 1: 2, 2: len(da.BLANK_GZIP_HEADER)}[wrapper]
            raise AssertionError("%s, wrapper %d: after flush %d (at %d) %d bytes, the oracle %d: %s" % (
                c["name"], wrapper, k, p, len(got), marks[k], fc.flush_diff(_closed(got[skip:]), _closed(ref[skip:marks[k]]), c, k)))
        if wrapper:
            assert enc.checksum() == sums[k], (c["name"], wrapper, k)
        k += 1
    got = enc.finish().getvalue()
    if got != ref:
        raise AssertionError("%s, wrapper %d: the finished stream has %d bytes, the oracle's %d: %s" % (
            c["name"], wrapper, len(got), len(ref), fc.flush_diff(got, ref, c) if wrapper == 0 else "(framed)"))
    assert zlib.decompress(got, {0: -15, 1: 15, 2: 31}[wrapper]) == data
    return got


def _closed(raw):
    """a flushed stream so far, ended so that it can be read: an empty final block behind the sync marker"""
    return raw + b"\x03\x00"


# ---- each case on a fresh context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.names())
def test_case_on_a_fresh_context(da, name):
    c = fc.case(name)
    ctx = da.Context(0)
    try:
        run_case(da, ctx, c)
        if c["claims"].get("q1_zero"):  # (the last call is a mid-stream one whose first block fills inside its first window)
            assert ctx.info()["q1_rewarm"] == 0
    finally:
        ctx.close()


FRAMED = ["cut_default_k0_1_2_3_4_15_16_17_257_258_259_F_on_m16_m256_m1024_m4096", "filing_skew_F65536_q65536",
          "window_n_e_first_x_32768_plus_4097_match_of_258_below_e_first_x_32768",
          "trim_hole_at_base_F65537_q65536", "blocks_seg_1_0_31743_31744_31745_tokens_flush_behind_a_full_block", "many_65_flushes_default"]


@pytest.mark.parametrize("name", FRAMED)
def test_one_case_of_each_family_as_zlib_and_gzip(da, name):
    """header, checksum() after every flush and the trailer around the same blocks"""
    assert {fc.family_of(n) for n in FRAMED} == set(fc.FAMILIES)
    c = fc.case(name)
    ctx = da.Context(0)
    try:
        raw = fc.oracle(c)[0]
        for wrapper in (1, 2):
            got = run_case(da, ctx, c, wrapper)
            assert raw in got
    finally:
        ctx.close()


# ---- all cases of a level in sequence on one context, then a plain call ---------------------------------------------------------------
LEVELS = sorted({fc.opts_of(n) for n in fc.names()})


@pytest.mark.parametrize("opts", LEVELS, ids=[fc.LEVEL_NAMES[o] for o in LEVELS])
def test_all_cases_of_a_level_on_one_context(da, opts):
    """lists, flush points and the Q1 state of one stream must not reach the next call of the context"""
    ctx = da.Context(0)
    try:
        last = None
        for n in fc.names():
            if fc.opts_of(n) == opts:
                last = fc.case(n)
                run_case(da, ctx, last)
        got = ctx.encode(last["data"], da.CompressionOptions(*opts))
        want = ob.encode(last["data"], opts=ob.make_opts(*opts))
        assert got == want, "a one-shot call behind the streams of %s: %s" % (fc.LEVEL_NAMES[opts], fc.flush_diff(got, want, dict(last, targets=[])))
        assert ctx.blocks() == ob.trace_blocks()
    finally:
        ctx.close()


# ---- the first piece of every cut case as a one-shot call that ends in a sync flush -----------------------------------------------------
@pytest.mark.parametrize("name", [n for n in fc.names() if fc.family_of(n) == "cut"])
def test_first_piece_of_a_cut_case_as_a_sync_call(da, name):
    c = fc.case(name)
    ref, marks, _ = fc.oracle(c)
    first = c["script"][0]
    assert c["script"][1] == "F"
    ctx = da.Context(0)
    try:
        got = ctx.encode(c["data"][:first], da.CompressionOptions(*c["opts"]), flush=MI355_FLUSH_SYNC)
    finally:
        ctx.close()
    want = ref[:marks[0]]
    assert got == want, fc.flush_diff(_closed(got), _closed(want), dict(c, targets=[]), 0)
    d = zlib.decompressobj(-15)
    assert d.decompress(got) == c["data"][:first] and got.endswith(b"\x00\x00\xff\xff")
