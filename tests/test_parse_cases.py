"""The inputs of tests/parse_cases.py on the CPU.  Every case must force what it is there for -- check() asserts its claims on
the model and the model's path and tokens per segment on the oracle --, the host build of stages.h with segments of 1024 and a
fan of 16 must give the oracle's bytes on every case with no mismatch between the hierarchical and the serial parse, the
trains must keep every case's steps, heads and tokens, and every mutant of the model (one rule of the kernels wrong) must change
the predicted outcome of at least one case.  With that, a failure of tests/test_parse_gpu.py on a case points at what only the
GPU runs.  CPU only."""
import zlib

import numpy as np
import pytest

import hostsim_binding as hs
import oracle_binding as ob
import parse_cases as pc


@pytest.mark.parametrize("name", pc.names())
def test_case_forces_what_it_is_there_for(name):
    pc.check(pc.case(name))


def test_stage_functions_agree_with_the_oracle():
    for n in pc.names():
        c = pc.case(n)
        ref = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
        rb = ob.trace_blocks()
        rc, out, flags, bl = hs.encode(c["data"], *c["opts"], 1024, 16)
        assert rc == 0 and not (flags & 4), (n, rc, flags)
        assert out == ref, "%s: %s" % (n, pc.parse_diff(out, ref, c))
        assert bl == rb, n
        assert zlib.decompress(ref, -15) == c["data"]


def test_families_cover_the_listed_values():
    cl = {n: pc.case(n)["claims"] for n in pc.names()}
    fam = lambda f: [n for n in pc.names() if pc.case(n)["family"] == f]
    assert {f for f in (pc.case(n)["family"] for n in pc.names())} == {"slot", "lazy", "adv", "seam", "runup", "repair"}
    for level in ("default", "lazy8"):
        got = {(cl[n]["chain"][1] % 4, cl[n]["chain"][0]) for n in fam("lazy") if n.startswith("lazy_%s_q" % level)}
        assert got == {(q, c) for q in range(4) for c in range(min(10, pc.LEVEL[level][1] - 2))}, level
    assert {cl[n]["chain"][0] for n in fam("adv") if "best" in n} == {29, 30, 31, 32, 33, 64, 125}
    assert {cl[n]["seam"][1] for n in fam("seam") if "seam" in cl[n] and "maxstep" not in n} == {0, 1, 2, 3, 127, 128, 129, 257, 258}
    # (the largest step of a level: lazy_if_less_than - 3 deferrals and a match of 258; the seam is one less)
    assert {n: cl[n]["seam"][1] for n in fam("seam") if "maxstep" in n} == {"seam_default_maxstep": 29 + 258 - 1, "seam_best_maxstep": 125 + 258 - 1}
    assert {(n.split("_")[1], cl[n]["far"][1]) for n in fam("lazy") if "far" in cl[n]} == {(lv, f) for lv in ("default", "lazy8") for f in (False, True)}
    assert {cl[n]["land"][1] - 4 * pc.SEG for n in fam("runup") if "land" in cl[n]} == {-1, 0, 1}
    assert {cl[n]["chain"][0] for n in fam("adv") if "lazy64" in n} == {29, 30, 31, 33, 61}
    assert {cl[n]["covered_last"] for n in fam("seam") if "covered_last" in cl[n]} == {1, 2, 3, 257}
    assert {cl[n]["run"] for n in fam("repair") if n.startswith("repair_default_r")} >= {1, 2, 3, 23, 24, 25}
    assert {cl[n]["heads_at"][0] for n in fam("repair") if n.startswith("heads_default_") and len(cl[n].get("heads_at", ())) == 1} >= {63, 64, 65, 255, 256, 257}
    over = {pc.model_of(pc.case(n))["tokens"][cl[n]["slot_seg"]] for n in fam("slot") if "slot_seg" in cl[n]}
    assert over >= {1024, 1025, 1026, 1024 + 29, 1023 + 29, 1024 + 125, 1023 + 125}, sorted(over)


@pytest.mark.parametrize("level,families", pc.TRAINS, ids=["%s-%s" % (a, b.replace(" ", "_")) for a, b in pc.TRAINS])
def test_train_keeps_every_case(level, families):
    tr = pc.train(level, families)
    m = pc.check_train(tr)
    assert len(tr["data"]) < (5 << 20) and m["K"] > pc.SMALL_SEGS


@pytest.mark.parametrize("nheads", [1023, 1024, 1025])
def test_fix_max_inputs_have_exactly_that_many_heads(nheads):
    c = pc.fixmax(nheads)
    m = pc.check(c)
    assert m["K"] > pc.SMALL_SEGS and len(c["data"]) < (5 << 20)
    assert len(m["heads"]) == nheads and m["bad"] == m["heads"] and m["fallback"] == (nheads > pc.FIX_MAX)


def test_the_steps_form_is_the_step_but_where_it_says_so():
    """the restatement of emit_body.inc:56-84 gives parse_step's length at every position of the lazy cases, or -1 (escalation)
    exactly at the chains with q + deferrals >= 8"""
    for n in pc.names():
        c = pc.case(n)
        if c["family"] != "lazy":
            continue
        adv, ntok, run, fromq = pc.steps_cached(c)
        got = pc.lazy_form(c)
        esc = got < 0
        assert np.array_equal(got[~esc], adv[~esc]), (n, int(np.argmax((got != adv) & ~esc)))
        j = np.arange(len(adv))
        assert np.array_equal(esc, (adv > 1) & (j % 4 + ntok - 1 >= 8)), n


# A mutant is the model with one rule wrong.  Each must change what the model predicts for at least one case.
def _outcome(c, **kw):
    m = pc.model_of(c, **kw)
    return (m["E"], m["heads"], m["still"], m["fallback"], sorted(m["hops"].items()))


MUTANTS = [
    ("a run-up of 127 positions", lambda c: _outcome(c, spec_w=127) != _outcome(c)),
    ("23 hops", lambda c: _outcome(c, hops=23) != _outcome(c)),
    ("FIX_MAX 1023", lambda c: _outcome(c, fix_max=1023) != _outcome(c)),
    ("a head test without the i == 1 branch", lambda c: _outcome(c, head_i1=False) != _outcome(c)),
    ("a nine-length window of eight", lambda c: c["family"] == "lazy" and not np.array_equal(pc.lazy_form(c, 8), pc.lazy_form(c))),
    ("ADV_RUN_MANY 30", lambda c: pc.escalated(c, 30) != pc.escalated(c)),
    ("a slot of 1023", lambda c: pc.over_slot(c, 1023) != pc.over_slot(c)),
]


@pytest.mark.parametrize("what,differs", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_mutant_of_the_model_is_caught(what, differs):
    cs = [pc.case(n) for n in pc.names()] + ([pc.fixmax(1024)] if what.startswith("FIX_MAX") else [])
    caught = [c["name"] for c in cs if differs(c)]
    print(what, len(caught), caught[:8])
    assert caught, "no case notices: %s" % what


def test_parse_diff_names_token_position_segment_and_the_model():
    c = pc.case("slot_default_c2_b1_middle")
    want = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
    assert pc.parse_diff(want, want, c) is None
    got = ob.encode(c["data"], opts=ob.make_opts(*pc.GREEDY))  # (no deferrals: the climb's first match is taken)
    msg = pc.parse_diff(got, want, c)
    s = c["claims"]["slot_seg"]
    assert "at input position %d (segment %d, byte 1023 of it)" % ((s + 1) * pc.SEG - 1, s) in msg and "tokens 1026" in msg, msg
