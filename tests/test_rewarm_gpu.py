"""The first-block re-warm (quirk Q1) on the GPU: the cases of tests/rewarm_cases.py through every entry point that evaluates the
predicate or runs the second pass, bit-exact against the oracle.  Every case puts the end of block 0, the two re-filed positions,
an identity hop or the hand-over from the link path to the sorted path where a kernel can be wrong by one (tests/test_rewarm_cases.py
asserts on the CPU that each case does, on the oracle alone, and that the host build of stages.h gives the oracle's stream): what is
left to go wrong is k_links_a / k_links_b / k_match with their re-filed lanes and identity entries, the device-side predicate, and
the drivers' bookkeeping.  On a mismatch rewarm_cases.rewarm_diff names the first differing token, its position and epoch, w, and
the model's chain for it.  pytest -m gpu."""
import io
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import datagen
import oracle_binding as ob
import rewarm_cases as rc

pytestmark = pytest.mark.gpu

SMALL = [n for n in rc.names() if rc.family_of(n) != "paths"]
# one case of every family for the other entry points
ONE_OF_EACH = ["predicate_default_match_ends_32768_fires", "filing_two_foreign_in_batch_below", "hop_default_after_slide_w32768",
               "handover_default_targets"]


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


def encode_and_compare(da, ctx, c, what=""):
    """one host call; the stream, the Q1 flag and the number of passes against the case's claims"""
    got = ctx.encode(c["data"], da.CompressionOptions(*c["opts"]))
    want = rc.oracle(c)
    assert got == want, "%s%s" % (what, rc.rewarm_diff(got, want, c))
    info = ctx.info()
    fires = c["claims"]["fires"]
    assert info["q1_rewarm"] == int(fires), (c["name"], what, info["q1_rewarm"])
    assert info["passes"] == (2 if fires else 1), (c["name"], what, info["passes"])
    return got


# ---- each case on a fresh context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_case_on_a_fresh_context(da, name):
    c = rc.case(name)
    ctx = da.Context(0)
    try:
        encode_and_compare(da, ctx, c)
        assert ctx.blocks() == rc.oracle_blocks(c)
    finally:
        ctx.close()


# ---- all cases of a level in sequence on one context, then a plain call and the twin that does not fire --------------------------------
LEVELS = sorted({rc.opts_of(n) for n in SMALL})


@pytest.mark.parametrize("opts", LEVELS, ids=[rc.LEVEL_NAMES[o] for o in LEVELS])
def test_all_cases_of_a_level_on_one_context(da, opts):
    """the re-warm of one call (q1_last_on, the override the second pass latched) must not reach the next call of the context"""
    ctx = da.Context(0)
    try:
        for n in SMALL:
            if rc.opts_of(n) == opts:
                encode_and_compare(da, ctx, rc.case(n), "in sequence: ")
        text = datagen.text_like(70000, 71)
        got = ctx.encode(text, da.CompressionOptions(*opts))
        want = ob.encode(text, opts=ob.make_opts(*opts))
        assert got == want, "a text call behind the cases of %s: %s" % (rc.LEVEL_NAMES[opts], rc.mc.match_diff(got, want))
        assert (ctx.info()["q1_rewarm"], ctx.info()["passes"]) == (0, 1)
        twin = rc.quiet_twin(opts)
        assert not twin["claims"]["fires"]
        encode_and_compare(da, ctx, twin, "the twin that does not fire, behind the text call: ")
        # and a stream written in pieces right behind a call that fired: it starts from the handle's own state
        fired = rc.case(next(n for n in SMALL if rc.opts_of(n) == opts and rc.case(n)["claims"]["fires"]))
        encode_and_compare(da, ctx, fired, "once more: ")
        enc = da.DeflateEncoder(io.BytesIO(), da.CompressionOptions(*opts), ctx=ctx)
        enc.write(text[:30000])
        enc.write(text[30000:])
        assert enc.finish().getvalue() == want, "a text stream behind a call that fired"
    finally:
        ctx.close()


# ---- one case of every family through the other entry points --------------------------------------------------------------------------
def test_one_of_each_names_every_family():
    assert {rc.family_of(n) for n in ONE_OF_EACH} | {"paths"} == set(rc.FAMILIES)
    assert all(rc.case(n)["claims"]["fires"] for n in ONE_OF_EACH)


@pytest.mark.parametrize("name", ONE_OF_EACH)
def test_device_call_on_torch_tensors(da, name):
    """mi355_deflate_encode_device: input and output in device memory"""
    c = rc.case(name)
    data, want = c["data"], rc.oracle(c)
    ctx = da.Context(0)
    try:
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        cap = da.bound(len(data)) + 16
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        n = ctx.encode_device(t.data_ptr(), len(data), out.data_ptr(), cap, da.CompressionOptions(*c["opts"]))
        got = bytes(out[:n].cpu().numpy())
        assert got == want, rc.rewarm_diff(got, want, c)
        assert (ctx.info()["q1_rewarm"], ctx.info()["passes"]) == (1, 2)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ONE_OF_EACH)
def test_zlib_and_gzip(da, name):
    """header and trailer around the same blocks: the checksum stages run beside both passes"""
    c = rc.case(name)
    data, opts = c["data"], c["opts"]
    raw = rc.oracle(c)
    ctx = da.Context(0)
    try:
        for wrapper in (1, 2):
            want = rc.oracle(c, 1) if wrapper == 1 else ob.encode_gzip(data, da.BLANK_GZIP_HEADER, opts=ob.make_opts(*opts, 0))
            got = ctx.encode(data, da.CompressionOptions(*opts), wrapper=wrapper)
            skip = 2 if wrapper == 1 else len(da.BLANK_GZIP_HEADER)
            assert got == want, "wrapper %d: %s" % (wrapper, rc.rewarm_diff(got[skip:], want[skip:], c))
            assert raw in got and ctx.info()["q1_rewarm"] == 1
            assert zlib.decompress(got, 15 if wrapper == 1 else 31) == data
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ONE_OF_EACH)
def test_stream_written_in_two_parts(da, name):
    """DeflateEncoder, the input split at 50 000 (one byte before its end where it is shorter) and at w: the never-flushed stream
    is one encode call over the bytes of both writes"""
    c = rc.case(name)
    data, want, w = c["data"], rc.oracle(c), c["claims"]["w"]
    assert 0 < w < len(data)
    ctx = da.Context(0)
    try:
        for cut in (min(50000, len(data) - 1), w):
            enc = da.DeflateEncoder(io.BytesIO(), da.CompressionOptions(*c["opts"]), ctx=ctx)
            enc.write(data[:cut])
            enc.write(data[cut:])
            got = enc.finish().getvalue()
            assert got == want, "written in two parts, cut at %d: %s" % (cut, rc.rewarm_diff(got, want, c))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ONE_OF_EACH)
def test_batch_with_the_case_in_the_middle_of_eight_texts(da, name):
    """encode_batch: the batch's first pass finds the full first block, the item goes through the single path, and the
    neighbours' streams are what they are alone"""
    c = rc.case(name)
    opts = c["opts"]
    texts = [datagen.text_like(9000 + 3001 * k, 80 + k) for k in range(8)]
    datas = texts[:4] + [c["data"]] + texts[4:]
    wants = [ob.encode(d, opts=ob.make_opts(*opts)) for d in texts]
    wants = wants[:4] + [rc.oracle(c)] + wants[4:]
    ctx = da.Context(0)
    try:
        gots = ctx.encode_batch(datas, da.CompressionOptions(*opts))
        assert gots[4] == wants[4], "item 4 of 9: %s" % rc.rewarm_diff(gots[4], wants[4], c)
        for k in range(9):
            assert gots[k] == wants[k], "item %d of 9 (a text beside the case): %s" % (k, rc.mc.match_diff(gots[k], wants[k]))
        bi = ctx.batch_info()
        assert bi["n_q1_single"] == 1 and bi["n_items"] == 9, bi
    finally:
        ctx.close()


# ---- the large path and the streamed host call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["paths_default_hop_large", "paths_two_filing_large"])
def test_large_path(da, name):
    """2 MiB + 1 KiB, 2 049 segments: k_block_bounds evaluates the predicate and stops the first pass's block stages (q1_cancel)"""
    c = rc.case(name)
    ctx = da.Context(0)
    try:
        encode_and_compare(da, ctx, c)
        data = c["data"]
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        cap = da.bound(len(data)) + 16
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        n = ctx.encode_device(t.data_ptr(), len(data), out.data_ptr(), cap, da.CompressionOptions(*c["opts"]))
        got = bytes(out[:n].cpu().numpy())
        assert got == rc.oracle(c), rc.rewarm_diff(got, rc.oracle(c), c)
        assert (ctx.info()["q1_rewarm"], ctx.info()["passes"]) == (1, 2)
    finally:
        ctx.close()


def test_streamed_host_call(da):
    """the smallest input that the host call works on piece by piece (run_streamed): its first piece finds the full first block,
    nothing has been handed out yet, and the call is made again in one"""
    c = rc.case("paths_default_hop_streamed")
    assert len(c["data"]) == rc.HOST_PIECEWISE_FROM
    ctx = da.Context(0)
    try:
        got = ctx.encode(c["data"], da.CompressionOptions(*c["opts"]))
        want = rc.oracle(c)
        assert got == want, rc.rewarm_diff(got, want, c)
        assert ctx.info()["q1_rewarm"] == 1
    finally:
        ctx.close()
