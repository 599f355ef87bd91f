"""The match walk on the GPU (k_match3, k_match3_both with and without SINGLE, kb_walk) on the inputs of tests/match_cases.py:
chains that put a probe hit into every slot of a group of eight behind real and false hits, end the own-epoch part of a bucket,
the window and the budget at every offset from the last hit, split the candidates of a small call's walk at every rank around
the middle, and reach every length and alignment of the 16-byte compare.  Each target's match is a token of the oracle's stream
(tests/test_match_cases.py asserts that on the CPU, and that the serial stage functions agree with the oracle on every case), so
a wrong table entry changes bytes: every stream here must equal the oracle's byte for byte, with its block table, and inflate to
the input.  A mismatch is reported by token, input position, target and the model's visits around the decisive rank.

The forms of the walk are chosen by the host (deflate_host.inc walk_plan / match3_split, restated in plan() below): a case alone is a
small call (split 16, SINGLE: near and far half), a batch is kb_walk, and the trains put all cases of a level behind a lead-in
whose length selects the both-tables kernel with whole epochs and the turn-round of the results through the LDS, k_match3 proper
with whole epochs, k_match3 in parts, and the both-tables kernel in 16 parts without SINGLE.  plan() is asserted for every train,
so a change of the thresholds fails the test instead of emptying it.

The permuted-table form (k_match3_swz, PairWinT<true>) is taken for epochs that k_sort marks; tests/test_match_walk_swz_gpu.py
runs these cases through it on the test build of the library, which can set the mark and reports it.  pytest -m gpu."""
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import match_cases as mc
import oracle_binding as ob

pytestmark = pytest.mark.gpu

OPTS = sorted({mc.opts_of(n) for n in mc.names()})
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


def oracle(c):
    """(stream, block table) of the oracle for a case or a train, made once"""
    if c["name"] not in _REF:
        ref = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
        _REF[c["name"]] = (ref, ob.trace_blocks())
    return _REF[c["name"]]


def same_stream(got, c, what):
    ref = oracle(c)[0]
    if got != ref:
        raise AssertionError("%s != oracle (%d vs %d bytes): %s" % (what, len(got), len(ref), mc.match_diff(got, ref, c)))


# ---- the host's rules, restated -------------------------------------------------------------------------------------------------------
plan = mc.plan  # (match_cases.py: shared with tests/test_match_walk_swz_gpu.py)


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- each case alone: a small call, k_match3_both<.., SINGLE> -------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.names())
def test_case_alone(da, ctx, name):
    c = mc.case(name)
    n_ep = (len(c["data"]) + mc.EPOCH - 1) // mc.EPOCH
    assert plan(n_ep, n_cu()) == (16, True, True), "a case alone is no longer a small call's walk"
    out = ctx.encode(c["data"], da.CompressionOptions(*c["opts"]), compat=1)
    bl = ctx.blocks()
    same_stream(out, c, "the walk of %s alone" % name)
    assert bl == oracle(c)[1]
    assert zlib.decompress(out, -15) == c["data"]


# ---- all cases of one set of options in one batch: kb_walk ----------------------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTS, ids=["%d_%d_%d" % o for o in OPTS])
def test_all_cases_of_a_level_in_one_batch(da, ctx, opts):
    cs = [mc.case(n) for n in mc.names() if mc.opts_of(n) == opts]
    o = da.CompressionOptions(*opts)
    outs = ctx.encode_batch([c["data"] for c in cs], o, compat=1)
    bi = ctx.batch_info()
    for k, (c, out) in enumerate(zip(cs, outs)):
        same_stream(out, c, "kb_walk on %s (item %d of the batch)" % (c["name"], k))
        assert zlib.decompress(out, -15) == c["data"]
    if opts[2] == 1 and opts[1] > 32 and opts[0] >> 2 == 0:
        # (a quarter budget of no checks: the batched call hands such items to the one-input path, deflate_batch.inc batch_takes)
        assert bi["n_items"] == bi["n_single"] == len(cs), bi
        return
    assert bi["n_items"] == len(cs) and bi["n_batched"] == len(cs), "an item left the launch set: kb_walk did not see it (%s)" % (bi,)
    # The same items from one device buffer, each behind an item of 1 .. 15 odd bytes, so that the inputs start on every residue
    # of 16: kb_walk with in_aligned16 == 0.  (The host call stages every item on a 256-byte boundary: device items stay in place.)
    arena, spans = bytearray(), []
    for k, c in enumerate(cs):
        arena += bytes(-len(arena) % 16)
        odd = bytes([65 + k % 15]) * (1 + k % 15)
        spans += [(len(arena), odd), (len(arena) + len(odd), c["data"])]
        arena += odd + c["data"]
    buf = torch.frombuffer(arena, dtype=torch.uint8).cuda()
    assert buf.data_ptr() % 16 == 0 and (len(cs) < 15 or {off % 16 for off, _ in spans[1::2]} == set(range(1, 16)))
    outs, lens, _ = ctx.encode_batch_device([(buf.data_ptr() + off, len(d)) for off, d in spans], None, o, compat=1)
    bi = ctx.batch_info()
    assert bi["n_items"] == len(spans) and bi["n_batched"] == len(spans), "an item left the launch set (%s)" % (bi,)
    torch.cuda.synchronize()
    for k, c in enumerate(cs):
        got = bytes(outs[2 * k + 1][:lens[2 * k + 1]].cpu().numpy())
        same_stream(got, c, "kb_walk on %s at residue %d (item %d)" % (c["name"], spans[2 * k + 1][0] % 16, 2 * k + 1))
        assert zlib.decompress(bytes(outs[2 * k][:lens[2 * k]].cpu().numpy()), -15) == spans[2 * k][1]


# ---- each case from a device buffer that begins 1, 3, 8 and 15 bytes behind a 16-byte boundary ----------------------------------------
@pytest.mark.parametrize("name", mc.names())
def test_case_from_an_unaligned_device_buffer(da, ctx, name):
    c = mc.case(name)
    data, o = c["data"], da.CompressionOptions(*c["opts"])
    cap = da.bound(len(data)) + 8
    buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    host = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for off in (1, 3, 8, 15):
        buf.zero_()
        buf[off:off + len(data)] = host.cuda()
        torch.cuda.synchronize()
        n = ctx.encode_device(buf.data_ptr() + off, len(data), out.data_ptr(), cap, o, compat=1)
        same_stream(bytes(out[:n].cpu().numpy()), c, "the walk of %s from a buffer at offset %d" % (name, off))


# ---- trains: all cases of a level behind a lead-in that selects the form of the walk ---------------------------------------------------
# SINGLE with 16 parts is what every case alone runs (test_case_alone asserts it); 16 parts without SINGLE needs 9 to 16 epochs at
# 256 compute units, which the two cases of Best behind four epochs of lead-in have.
@pytest.mark.parametrize("level,epochs,lead,want,form", mc.TRAIN_FORMS, ids=["%s_%s_%s" % t[:3] for t in mc.TRAIN_FORMS])
def test_train(da, ctx, level, epochs, lead, want, form):
    tr = mc.train_of(level, epochs, lead)
    n_ep = len(tr["data"]) // mc.EPOCH
    got = plan(n_ep, n_cu())
    print(tr["name"], "epochs", n_ep, "n_cu", n_cu(), "(split, single, both) =", got, "--", form)
    assert n_ep == epochs and len(tr["data"]) < (16 << 20)
    assert got == want, "%s: %d epochs on %d compute units give %s, not %s" % (form, n_ep, n_cu(), got, want)
    out = ctx.encode(tr["data"], da.CompressionOptions(*tr["opts"]), compat=1)
    bl = ctx.blocks()
    same_stream(out, tr, "the walk of %s (%s)" % (tr["name"], form))
    assert bl == oracle(tr)[1]
    assert zlib.decompress(out, -15) == tr["data"]


# ---- the small trains with ballot ranks in the sort: ties depend on the order in the bucket --------------------------------------------
@pytest.mark.parametrize("level,lead", mc.SMALL_TRAINS)
def test_small_train_with_ballot_ranks(da, level, lead):
    tr = mc.train(level, 2, lead)
    c = da.Context(0)
    try:
        c.config(c.CFG_SORT_RANKS, 0)
        out = c.encode(tr["data"], da.CompressionOptions(*tr["opts"]), compat=1)
        bl = c.blocks()
    finally:
        c.close()
    same_stream(out, tr, "the walk of %s, ballot ranks" % tr["name"])
    assert bl == oracle(tr)[1]
    assert zlib.decompress(out, -15) == tr["data"]
