"""The parse on the GPU (k_emit<0|1|2> with emit_body.inc, k_spec_check, k_small_fix, k_scan_a, k_compact, the exact way through
k_seg_exit / k_level_up / k_level_down / k_tree_top, kb_emit and kb_small_fix) on the inputs of tests/parse_cases.py: seams with
the previous segment left 0 to 258 and, by the levels' largest steps, 286 (Default) and 382 (Best) bytes into the next, run-ups that merge at their first and last position, runs of
1 to 25 failed boundaries, heads on the edges of the ballot word, the badmap word and the k_spec_check workgroup, 1023 / 1024 /
1025 heads, chains of 0 to 9 deferrals at every position mod 4 and the levels' longest, and segments of 1024 to 1024 + 125 tokens.
tests/test_parse_cases.py asserts on the CPU that every case forces what its name says and that the serial stage functions agree
with the oracle on it, so a failure here points at what only the GPU runs.  In every form the stream, the block table and the
inflated bytes must equal the oracle's, and what the call reports about its speculation must be the model's: spec_repaired is
the number of heads (0 after a fallback: the call is run again with a cleared state), spec_fallback is 0 exactly where the
repair closes every boundary.  A mismatch is reported by token, input position, segment and the model's entries and exits.

The token slot.  A segment's tokens are those of the steps that start in it, so a segment of literals that ends in a chain of c
deferrals holds 1024 + c tokens (family `slot`; `seam_*_maxstep`, `lazy_default_front*` and `runup_default_chain` have such
segments as well).  By the code, a slot of SEG words cannot hold them: the tokens behind the 1024th land in the first words of
the next segment's slot, which that segment's own wave writes, and k_compact and token_start read one of the two wrong.  The
slot is TOK_SLOT = SEG + 256 words (deflate_kernels.hip), which bounds the longest lazy step behind SEG - 1 literals.
pytest -m gpu."""
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import oracle_binding as ob
import parse_cases as pc

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


def oracle(c):
    """(stream, block table) of the oracle for a case or a train, made once"""
    if c["name"] not in _REF:
        ref = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
        _REF[c["name"]] = (ref, ob.trace_blocks())
    return _REF[c["name"]]


def same_as_oracle(out, bl, c, what):
    ref, rb = oracle(c)
    if out != ref:
        raise AssertionError("%s != oracle (%d vs %d bytes): %s" % (what, len(out), len(ref), pc.parse_diff(out, ref, c)))
    assert bl is None or bl == rb, what
    assert zlib.decompress(out, -15) == c["data"], what


def reports_the_model(info, c, what):
    m = pc.model_of(c)
    print(what, "heads", len(m["heads"]), "still", len(m["still"]), "-> spec_repaired", info["spec_repaired"], "spec_fallback", info["spec_fallback"])
    assert info["spec_repaired"] == m["repaired"], (what, info["spec_repaired"], m["heads"][:8], m["fallback"])
    assert (info["spec_fallback"] >= 1) == m["fallback"], (what, info["spec_fallback"], m["still"][:8])


# ---- each case alone on a fresh context: the small call, k_small_fix, with the steps from k_emit and from k_adv ------------------------
@pytest.mark.parametrize("name", pc.names())
def test_case_alone(da, name):
    c = pc.case(name)
    assert pc.model_of(c)["K"] <= pc.SMALL_SEGS
    for where in (1, 0):
        ctx = da.Context(0)
        try:
            ctx.config(da.Context.CFG_STEPS_IN_EMIT, where)
            out = ctx.encode(c["data"], da.CompressionOptions(*c["opts"]), compat=1)
            bl, info = ctx.blocks(), ctx.info()
        finally:
            ctx.close()
        what = "%s alone, CFG_STEPS_IN_EMIT %d" % (name, where)
        same_as_oracle(out, bl, c, what)
        reports_the_model(info, c, what)


# ---- trains: K above 2048 -- k_emit<1>, k_spec_check, k_emit<2>, k_scan_a, k_compact --------------------------------------------------
TRAINS = [(lv, fam, None) for lv, fam in pc.TRAINS] + [("default", "fixmax", h) for h in (1023, 1024, 1025)]


@pytest.mark.parametrize("level,families,extra", TRAINS, ids=["%s-%s-%s" % (a, b.replace(" ", "_"), e) for a, b, e in TRAINS])
def test_train(da, level, families, extra):
    tr = pc.train(level, families, extra)
    m = pc.model_of(tr)
    assert m["K"] > pc.SMALL_SEGS and len(tr["data"]) < (5 << 20)
    if extra:
        assert len(m["heads"]) == extra and m["fallback"] == (extra > pc.FIX_MAX)
    ctx = da.Context(0)
    try:
        out = ctx.encode(tr["data"], da.CompressionOptions(*tr["opts"]), compat=1)
        bl, info = ctx.blocks(), ctx.info()
    finally:
        ctx.close()
    same_as_oracle(out, bl, tr, tr["name"])
    reports_the_model(info, tr, tr["name"])


# ---- the exact way: behind a call that fell back the context parses with exit tables and the tree ---------------------------------------
def test_exact_way_behind_a_fallback_and_speculation_after_the_pause(da):
    first = pc.case("repair_default_r25")
    witness = [pc.case(n) for n in ("repair_default_r3", "repair_default_r24", "heads_default_64", "runup_default_merge_behind",
                                   "seam_default_maxstep", "seam_default_d257", "slot_default_c29_b1_middle")]
    assert pc.model_of(first)["fallback"] and all(not pc.model_of(c)["fallback"] for c in witness)
    assert sum(1 for c in witness if pc.model_of(c)["heads"]) >= 4
    calls = [pc.exact(K) for K in pc.EXACT_K] + witness
    assert len(calls) == pc.EXACT_CALLS
    ctx = da.Context(0)
    try:
        o = da.CompressionOptions(*pc.DEFAULT)
        out = ctx.encode(first["data"], o, compat=1)
        same_as_oracle(out, ctx.blocks(), first, "the call that falls back")
        assert ctx.info()["spec_fallback"] >= 1
        for c in calls:
            out = ctx.encode(c["data"], o, compat=1)
            bl, info = ctx.blocks(), ctx.info()
            same_as_oracle(out, bl, c, "%s the exact way" % c["name"])
            # (the witness that the tree ran: nothing was checked, nothing repaired)
            assert info["spec_repaired"] == 0 and info["spec_fallback"] == 0, (c["name"], info["spec_repaired"], info["spec_fallback"])
        back = witness[0]
        out = ctx.encode(back["data"], o, compat=1)
        same_as_oracle(out, ctx.blocks(), back, "%s after the pause" % back["name"])
        reports_the_model(ctx.info(), back, "speculation is back")
        assert ctx.info()["spec_repaired"] == len(pc.model_of(back)["heads"]) > 0
    finally:
        ctx.close()


# ---- all cases of a level in one batch: kb_emit, kb_small_fix -----------------------------------------------------------------------------
BATCH_OPTS = sorted({pc.opts_of(n) for n in pc.names()})


@pytest.mark.parametrize("opts", BATCH_OPTS, ids=["%d_%d_%d" % o for o in BATCH_OPTS])
def test_all_cases_of_a_level_in_one_batch(da, opts):
    cs = [pc.case(n) for n in pc.names() if pc.opts_of(n) == opts]
    ctx = da.Context(0)
    try:
        outs = ctx.encode_batch([c["data"] for c in cs], da.CompressionOptions(*opts), compat=1)
        bi = ctx.batch_info()
    finally:
        ctx.close()
    for k, (c, out) in enumerate(zip(cs, outs)):
        same_as_oracle(out, None, c, "%s, item %d of the batch" % (c["name"], k))
    fall = sum(1 for c in cs if pc.model_of(c)["fallback"])
    print(opts, len(cs), "items,", fall, "fall back:", {k: bi[k] for k in ("n_items", "n_batched", "n_single", "n_q1_single", "n_spec_single")})
    assert bi["n_items"] == len(cs) and bi["n_spec_single"] == fall, bi
    # (block 0 of slot_*_block0 fills inside the first window: quirk Q1 sends that item through the one-input path as well)
    assert bi["n_q1_single"] <= sum(1 for c in cs if "block0" in c["claims"]), bi
    assert bi["n_single"] == bi["n_spec_single"] + bi["n_q1_single"] and bi["n_batched"] == len(cs) - bi["n_single"], bi
