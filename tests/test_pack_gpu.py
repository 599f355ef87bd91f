"""plan_blocks (k_plan, kb_plan) and the pack (k_pack<1024>, k_pack<256>, kb_pack, fed by k_block_hist) on the inputs of
tests/pack_cases.py: blocks whose type hangs on the bit phase they start at, groups of stored blocks at every phase, sync
markers, stored payloads at every alignment, parts and rounds that end on a word boundary, headers of more than 256
run-coded lengths -- cases the other parity tests' inputs never reach (tests/test_pack_cases.py asserts on the CPU that
these do, and that the serial stage functions agree with the oracle on them).  Every comparison is byte for byte against
the oracle; a mismatch is reported by block, part and first differing bit.  pytest -m gpu."""
import io
import os
import sys
import zlib
from collections import Counter

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import oracle_binding as ob
import pack_cases as pc

pytestmark = pytest.mark.gpu

BATCH_ITEM_MAX = 2 << 20  # what a batch's launch set takes (SMALL_TAIL_SEGS segments)
ONE_SHOT = [n for n in pc.names() if "cuts" not in pc._CASES[n]]
SYNC = [n for n in pc.names() if "cuts" in pc._CASES[n]]
_REF = {}


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


def oracle(name):
    """(stream, block table) of the oracle, made once per case or train"""
    if name not in _REF:
        c = pc.case(name)
        _REF[name] = pc.oracle(c["data"], c["level"])
    return _REF[name]


def same_stream(got, ref, what):
    if got != ref:
        raise AssertionError("%s != oracle: %s" % (what, pc.pack_diff(got, ref)))


def one_input(da, ctx, name, what):
    c = pc.case(name)
    ref, rb = oracle(name)
    out = ctx.encode(c["data"], da.CompressionOptions(*pc.LV[c["level"]]), compat=1)
    bl, info = ctx.blocks(), ctx.info()
    same_stream(out, ref, "%s of %s" % (what, name))
    diff = next((i for i, (a, b) in enumerate(zip(bl, rb)) if a != b), None)
    assert bl == rb, "block table of %s: block %s is %s, expected %s" % (name, diff, bl[diff] if diff is not None else len(bl),
                                                                        rb[diff] if diff is not None else len(rb))
    assert zlib.decompress(out, -15) == c["data"]
    kinds = Counter(b["btype"] for b in rb)
    assert (info["n_stored"], info["n_fixed"], info["n_dynamic"], info["n_blocks"]) == (kinds[0], kinds[1], kinds[2], len(rb)), info
    return out, info


@pytest.mark.parametrize("name", [n for n in ONE_SHOT if n not in ("plain_1024", "plain_1025")])
def test_alone_in_a_fresh_context(da, name):
    """a one-input call of its own: up to 64 blocks it launches k_block_hist<1024> and k_pack<1024>"""
    c = da.Context(0)
    try:
        one_input(da, c, name, "one-input call")
    finally:
        c.close()


@pytest.mark.parametrize("name", pc.train_names() + ["plain_1024", "plain_1025"])
def test_train_in_one_call(da, ctx, name):
    """65 blocks and more in one call: k_block_hist<256> and k_pack<256> meet every member"""
    _, info = one_input(da, ctx, name, "train")
    assert info["n_blocks"] * 4 > 256


def test_streamed_input_piece_by_piece(da):
    """the plan per piece of the piece-wise host path: identical bytes with CFG_HOST_STREAMING 1 (two streams), 2 (one
    stream) and 0 (one piece), equal to the oracle's"""
    data = pc.streamed_input()
    ref = ob.encode(data, opts=ob.make_opts(*pc.LV["fast"]))
    rb = ob.trace_blocks()
    assert Counter(b["btype"] for b in rb)[0] > 64 and Counter(b["btype"] for b in rb)[2] > 64
    c = da.Context(0)
    try:
        for mode in (1, 2, 0):
            c.config(da.Context.CFG_HOST_STREAMING, mode)
            out = c.encode(data, da.CompressionOptions(*pc.LV["fast"]), compat=1)
            info = c.info()
            print("CFG_HOST_STREAMING", mode, "host_path", info["host_path"], "blocks", info["n_blocks"])
            same_stream(out, ref, "CFG_HOST_STREAMING %d" % mode)
            assert c.blocks() == rb
            assert bool(info["host_path"] & 1) == (mode != 0), "the call did not go (or went) piece by piece: %s" % info
    finally:
        c.close()


def _units_hi(n):
    return (n // pc.B + 3) * 4


def _units_lo(n):
    return (n // pc.B + 1) * 4


def _batch(da, ctx, level, names, fillers, what):
    datas = [pc.case(n)["data"] for n in names] + fillers
    opts = da.CompressionOptions(*pc.LV[level])
    outs = ctx.encode_batch(datas, opts, compat=1)
    bi = ctx.batch_info()
    print(what, level, len(names), "cases,", len(fillers), "fillers:", bi)
    # (no item leaves the launch set but those the Q1 rule sends out: none at these levels, which do not hash)
    assert bi["n_items"] == len(datas) and bi["n_single"] == bi["n_q1_single"] == bi["n_spec_single"] == 0, bi
    assert bi["n_batched"] == len(datas), "an item left the launch set: kb_plan / kb_pack did not see it"
    for k, (n, d, o) in enumerate(zip(names, datas, outs)):
        same_stream(o, oracle(n)[0], "%s: item %d (%s) of the batch" % (what, k, n))
        assert o == ctx.encode(d, opts, compat=1), n
        assert zlib.decompress(o, -15) == d
    for d, o in zip(fillers, outs[len(names):]):
        assert zlib.decompress(o, -15) == d


@pytest.mark.parametrize("level", pc.levels())
def test_batches_of_a_level(da, ctx, level):
    """all cases of a level that a launch set takes: in batches of at most 256 pack workgroups (kb_pack<1024>), then all in
    one batch with plain items added, above 256 (kb_pack<256>)"""
    names = [n for n in ONE_SHOT if pc._CASES[n]["level"] == level and len(pc.case(n)["data"]) <= BATCH_ITEM_MAX]
    assert names
    small, cur, units = [], [], 0
    for n in names:
        u = _units_hi(len(pc.case(n)["data"]))
        if u > 256:
            continue  # (too many blocks for a batch that small: the large batch has it)
        if units + u > 256:
            small.append(cur)
            cur, units = [], 0
        cur.append(n)
        units += u
    small.append(cur)
    for k, chunk in enumerate(small):
        _batch(da, ctx, level, chunk, [], "small batch %d" % k)
    fillers = [pc.Ts(range(s, s + 8))[:-5 - s] for s in range(9)]
    assert sum(_units_lo(len(pc.case(n)["data"])) for n in names) + sum(_units_lo(len(f)) for f in fillers) > 256
    _batch(da, ctx, level, names, fillers, "large batch")


@pytest.mark.parametrize("name", SYNC)
@pytest.mark.parametrize("wrapper", [0, 1])
def test_sync_markers_through_the_writers(da, ctx, name, wrapper):
    """DeflateEncoder and ZlibEncoder: what the writer holds behind every flush is what the oracle's stream object holds"""
    c = pc.case(name)
    cls = (da.DeflateEncoder, da.ZlibEncoder)[wrapper]
    sink = io.BytesIO()
    enc = cls(sink, da.CompressionOptions(*pc.LV[c["level"]]), ctx)
    ref = ob.Stream(ob.make_opts(*pc.LV[c["level"]], wrapper))
    prev = 0
    for k, cut in enumerate(c["cuts"]):
        enc.write_all(c["data"][prev:cut])
        ref.write_all(c["data"][prev:cut])
        enc.flush()
        ref.flush()
        got, want = sink.getvalue(), ref.output()
        assert got.endswith(b"\x00\x00\xff\xff")
        if got != want:
            raise AssertionError("behind flush %d (at byte %d): %s" % (k, cut, pc.pack_diff(got[2 * wrapper:], want[2 * wrapper:])))
        prev = cut
    enc.write_all(c["data"][prev:])
    ref.write_all(c["data"][prev:])
    got, want = enc.finish().getvalue(), ref.finish()
    assert got == want, pc.pack_diff(got[2 * wrapper:], want[2 * wrapper:])
    assert (zlib.decompress(got) if wrapper else zlib.decompress(got, -15)) == c["data"]
