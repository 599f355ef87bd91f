"""The inputs of tests/match_cases.py on the CPU.  Every case must force what it is there for -- asserted on the oracle alone:
the oracle's token at every target is the model's and the declared one, the ranks, gaps and distances the case claims are
read off the model's visit list, a budget claim changes the oracle's token with one check less -- the families must cover the
listed values, every mutant of the model (a walk with one thing wrong) must change the prediction for a target of the family
that is there to catch it, and the host build of stages.h (tests/hostsim) must give the model's table entry at every target
and the oracle's bytes in all formulations of the walk.  With that, a failure of tests/test_match_walk_gpu.py on the same case
points at what only the GPU runs: the step block, the staging of the window, the turn-round of the results.  CPU only."""
import zlib

import pytest

import hostsim_binding as hs
import match_cases as mc
import oracle_binding as ob


@pytest.mark.parametrize("name", mc.names())
def test_case_forces_what_it_is_there_for(name):
    mc.check(mc.case(name))


def _in_train(level):
    return sum(len(mc.case(n)["targets"]) for n in mc.names() if mc.opts_of(n) == mc.TRAINS[level] and mc.in_train(mc.case(n)))


@pytest.mark.parametrize("level,lead", mc.SMALL_TRAINS)
def test_small_train_keeps_every_target(level, lead):
    assert mc.check_train(mc.train(level, 2, lead)) == _in_train(level)


@pytest.mark.parametrize("level,epochs,lead", [t[:3] for t in mc.TRAIN_FORMS], ids=["%s_%s_%s" % t[:3] for t in mc.TRAIN_FORMS])
def test_train_keeps_every_target(level, epochs, lead):
    tr = mc.train_of(level, epochs, lead)
    assert len(tr["data"]) == epochs * mc.EPOCH
    assert mc.check_train(tr) == _in_train(level)


def test_every_listed_value_is_covered():
    r = lambda a, b: set(range(a, b + 1))
    cov = {f: mc.covered(f) for f in mc.FAMILIES}
    c = cov["gap"]
    assert c["opts"] == {mc.DEFAULT, mc.GREEDY}
    for n in ("gap_default", "gap_greedy"):  # (every value at both)
        cl = [t["claims"] for t in mc.case(n)["targets"]]
        assert {x["first"] for x in cl} == r(0, 17) and {x["gap"] for x in cl} == r(0, 33)
    c = cov["false_then_real"]
    pairs = {(t["claims"]["false"][0], t["claims"]["real"]) for n in mc.names() for t in mc.case(n)["targets"]
             if mc.case(n)["family"] == "false_then_real" and len(t["claims"]["false"]) == 1 and "real" in t["claims"]}
    assert pairs == {(i, j) for j in range(16) for i in range(j)}
    counts = {len(t["claims"]["false"]) for n in mc.names() for t in mc.case(n)["targets"] if "false" in t["claims"]}
    assert counts == {1, 2, 3} and c["false_last"] == {True}
    c = cov["own_end"]
    ends = {}
    for n in mc.names():
        for t in mc.case(n)["targets"]:
            if "variant" in t["claims"]:
                ends.setdefault(t["claims"]["variant"], set()).add(t["claims"].get("own_end"))
    assert ends == {"epoch0": r(0, 16), "empty_prev": r(0, 16), "prev_decisive": r(0, 16), "n1_zero": {None}}
    assert c["prev_rank"] == r(0, 16) and 0 in c["n1"]
    c = cov["window"]
    assert c["dist"] == {32767, 32768} and c["beyond"] == {32769} and c["win_last"] == r(0, 16) and c["p_abs"] == {32768, 32769}
    assert {k % 8 for k in c["win_last"]} == r(0, 7)
    c = cov["budget"]
    assert {o[0] for o in c["opts"]} == set(mc.BUDGETS) and c["longer_at"] == set(mc.BUDGETS)
    assert c["n1"] == {16 - k for k in (1, 3, 8)} and c["side"] == {-1, 0, 1, "tie", "far_longer"}
    assert c["half"] == {8, 64, 884} and c["decisive"] >= {h + s for h in (8, 64, 884) for s in (-1, 0, 1)}
    c = cov["quarter"]
    assert c["opts"] == {mc.BEST, (6, 64, 1), (3, 64, 1)} and c["q"] == {442, 1, 0}
    assert c["q_side"] == {-2, -1, 0, 1} and c["prev_length"] <= r(32, 127) and c["q_variant"] == {"plain", "hits", "no_hit_behind", "prev_epoch"}
    c = cov["length"]
    assert c["length"] >= set(mc.LENGTHS) and c["beyond_max"] == {True} and c["left"] == set(mc.LEFT) | {1, 2}
    al = {(t["claims"]["p16"], t["claims"]["q16"]) for n in mc.names() for t in mc.case(n)["targets"] if "p16" in t["claims"]}
    assert al == {(i, j) for i in range(16) for j in range(16)}
    c = cov["ties"]
    assert c["equal"] == {2, 3} and c["where"] == {"group", "seam", "batch64"}
    c = cov["run_mix"]
    assert c["run_pieces"] == {40} and {"first", "gap", "false", "real", "own_end"} <= set(c) and c["dist"] == {1}
    assert c["run_break"] == {4, 5, 18, 33, 101, 257, 258} and c["run_edge"] == {300, 5} and 0 in c["epoch_pos"] and min(c["epoch_pos"]) < 0
    c = cov["tail"]
    assert c["J"] == {1, 2, 3, 4} | set(mc.TAIL_J) and c["whole"] == {3, 4, 5, 6} and c["last64"] == {True}
    assert {j % 64 for j in mc.TAIL_J} == {63, 0, 1} and {j // 64 for j in mc.TAIL_J} >= {0, 1, 8}
    assert set(mc.FAMILIES) == {mc.case(n)["family"] for n in mc.names()}


# A mutant is the model with one thing wrong.  Each must change the predicted token of at least one target of the family it
# belongs to: a family that no mutant can disturb is not testing its edge.  (The family `tail` has none: its edge is the number
# of entries of the last sorted epoch, which is no part of the model; its claims J and last64 pin it.)
MUTANTS = [
    ("budget + 1", "budget", dict(d_checks=1)),
    ("budget - 1", "budget", dict(d_checks=-1)),
    ("window 32 767", "window", dict(window=32767)),
    ("window 32 769", "window", dict(window=32769)),
    ("a false hit ends the walk", "false_then_real", dict(mutant="false_hit_ends")),
    ("resume one entry late after a hit", "gap", dict(mutant="resume_late")),
    ("resume one entry late after a hit", "false_then_real", dict(mutant="resume_late")),
    ("resume one entry late after a hit", "own_end", dict(mutant="resume_late")),
    ("resume one entry late after a hit", "run_mix", dict(mutant="resume_late")),
    ("a false hit ends the walk", "run_mix", dict(mutant="false_hit_ends")),
    ("maxlen 257", "run_mix", dict(maxlen=257)),
    ("resume one entry early after a hit", "budget", dict(mutant="resume_early")),
    ("farthest among equals", "ties", dict(mutant="farthest_among_equals")),
    ("quarter + 1", "quarter", dict(d_quarter=1)),
    ("quarter - 1", "quarter", dict(d_quarter=-1)),
    ("maxlen 257", "length", dict(maxlen=257)),
    ("the far half wins ties", "budget", dict(far_wins_ties=True)),
]


@pytest.mark.parametrize("what,family,kw", MUTANTS, ids=["%s-%s" % (m[1], m[0].replace(" ", "_")) for m in MUTANTS])
def test_mutant_of_the_model_is_caught(what, family, kw):
    caught = []
    for n in mc.names():
        c = mc.case(n)
        if c["family"] == family:
            caught += [(n, t["p"]) for t in c["targets"] if mc.predict(c["data"], t, c["opts"], **kw) != (t["at"], t["tok"])]
    print(what, len(caught), caught[:6])
    assert caught, "no target of family %s notices: %s" % (family, what)


def test_host_build_gives_the_model_at_every_target():
    """hs.match_table (the serial walk of stages.h, the budget of the case) at every target whose walk starts from no match"""
    for n in mc.names():
        c = mc.case(n)
        table = hs.match_table(c["data"], c["opts"][0])
        for t in c["targets"]:
            if t["prev"] != (0, 0):
                continue
            (ln, d), _ = mc.walk(c["data"], t["p"], c["opts"][0])
            want = (ln, d)
            got = table[t["p"]]
            assert (got & 0xFFFF, got >> 16) == want, (n, t["p"], hex(got), want)


@pytest.mark.parametrize("mode", [0, 6, 7, 8])
def test_stage_functions_agree_with_the_oracle(mode):
    try:
        hs.use_multi(mode)
        for n in mc.names():
            c = mc.case(n)
            ref = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
            rb = ob.trace_blocks()
            rc, out, flags, bl = hs.encode(c["data"], *c["opts"], 1024, 4)
            assert rc == 0 and not (flags & 4), (n, rc, flags)
            assert out == ref, "%s, walk mode %d: %s" % (n, mode, mc.match_diff(out, ref, c))
            assert bl == rb, n
            assert zlib.decompress(ref, -15) == c["data"]
    finally:
        hs.use_multi(0)


def test_match_diff_names_token_position_and_target():
    """what a failing parity test prints: the first differing token, its position, the target and its visits"""
    c = mc.case("gap_default")
    want = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
    assert mc.match_diff(want, want, c) is None
    t = c["targets"][5]
    got = ob.encode(c["data"], opts=ob.make_opts(t["claims"]["first"] + 1, 32, 1))  # a budget that ends on this target's first hit
    msg = mc.match_diff(got, want, c)
    first = min(u["p"] for u in c["targets"] if u["claims"]["first"] + 1 + u["claims"]["gap"] >= t["claims"]["first"] + 1)
    assert ("input position %d:" % first) in msg and "expected ('ld', 9," in msg and "target at %d of gap_default" % first in msg, msg
