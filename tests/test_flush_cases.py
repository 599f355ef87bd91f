"""The streams of tests/flush_cases.py on the CPU.  Every case must force what it is there for -- asserted on the oracle alone: the
oracle's token at every target is the model's, a `changes` claim differs from the oracle's token under plain writes, an `unchanged`
claim does not, a `cut` claim has the length the flush point leaves; every quirk kind changes a token in every part of a stream it
can reach, every listed edge has a case, and every mutant of the model (one rule of the write calls wrong) predicts another token
than the oracle emits for a case of the family that is there to catch it.  With that, a failure of tests/test_flush_gpu.py on the
same case points at the library: the lists the stream handle derives, or the kernels that read them.  CPU only."""
import pytest

import flush_cases as fc


@pytest.mark.parametrize("name", fc.names())
def test_case_forces_what_it_is_there_for(name):
    fc.check(fc.case(name))


def test_every_quirk_kind_changes_a_token_where_it_can():
    cov = fc.covered()
    want = {(k, w) for k in ("hole", "skew") for w in ("first", "mid", "trim")} | {(k, "first") for k in ("rewarm", "early", "moved")}
    assert want <= cov, want - cov
    # a ghost -- a target whose own hash is the foreign hash of the late-filed position -- for every kind that files a position late
    ghosts = {t["kind"]: t["claim"] for c in fc.cases() for t in c["targets"] if t.get("ghost") and c["family"] == "filing"}
    assert ghosts == {"skew": "changes", "rewarm": "changes", "moved": "changes", "early": "unchanged"}, ghosts
    # and for the late filing at the base of a trim, whose foreign hash is the hash of its own three bytes: the copy finds it
    own = [t for t in fc.case("trim_skew_at_base_own_hash_F65536_q65536")["targets"]]
    assert [(t["p"], t["q"], t["claim"]) for t in own] == [(98304, 65536, "unchanged")]


EDGES = {
    "cut": ["k0_1_2_3_4_15_16_17_257_258_259", "default", "fast", "best", "greedy", "rle", "defer_F_minus_3", "_F_minus_2",
            "best_behind_a_match_of_40", "_m16", "_m256", "_m1024", "_m4096", "_m32768"],
    "filing": ["hole_F", "skew_F", "skew_ghost", "rewarm_F3_", "rewarm_F32767_", "rewarm_F32768_", "rewarm_F32769_", "fn65793", "fn65794",
               "early_F1_", "early_F2_", "early_F2_ghost", "moved_F20000_gap1", "gap2", "moved_ghost", "rewarm_ghost", "two_byte_write"],
    "window": ["dist32767", "dist32768", "dist32769", "mod32767", "mod0", "mod1", "e_first_x_32768_minus_1", "e_first_x_32768_plus_1",
               "e_first_x_32768_plus_4095", "e_first_x_32768_plus_4096", "e_first_x_32768_plus_4097", "match_of_258_below_e_first_x_32768", "per3_whole_stream_F65535",
               "per3_whole_stream_F65536"],
    "trim": ["emitted98303", "emitted98304", "emitted98305", "emitted131071", "emitted131072", "hole_at_base_F", "skew_at_base_F",
             "hole_at_base_minus_1", "skew_at_base_minus_1", "skew_at_base_own_hash", "literal_stretch_behind_base_no_q1", "q_at_base", "q_at_base_plus_1",
             "q_at_emitted_minus_32768"],
    "blocks": ["seg_1_0_31743_31744_31745_tokens", "flush_behind_a_full_block", "2x31744_tokens"],
    "many": ["many_%d_flushes_%s" % (m, lv) for m in fc.MANY for lv in ("default", "rle")],
}


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_every_listed_edge_has_a_case(family):
    mine = [n for n in fc.names() if fc.family_of(n) == family]
    for edge in EDGES[family]:
        assert any(edge in n for n in mine), "no case of %s for %s" % (family, edge)
    cs = [fc.case(n) for n in mine]
    if family == "cut":
        ts = [t for c in cs for t in c["targets"] if "mod" in t]
        for c in cs:
            if "k0_1" in c["name"]:
                assert [t["k"] for t in c["targets"]] == list(fc.CUT_K), c["name"]
        assert {t["mod"] for t in ts} == {(m, r) for m in fc.MODS for r in (0, 1, -1)}
        for c in cs:  # (the flush point of every target is where its residue says)
            calls = fc.replay(c["script"])
            for t in c["targets"]:
                if "mod" in t:
                    F = t["p"] + t["k"]
                    assert any(s["end"] == F for s in calls[:-1]) and (F - t["mod"][1]) % t["mod"][0] == 0, (c["name"], t)
    if family == "trim":
        assert {w for c in cs for w in c["claims"].get("q_at", ())} == {"base", "base+1", "emitted-32768"}
        assert {(c["claims"]["emitted"], c["claims"]["base"]) for c in cs if "emitted" in c["claims"]} == {
            (98303, 0), (98304, 65536), (98305, 65536), (131071, 65536), (131072, 98304)}
    if family == "window":
        assert {(t["qmod"], t["p"] - t["q"]) for c in cs for t in c["targets"] if "qmod" in t} == {
            (m, d) for m in (32767, 0, 1) for d in (32767, 32768, 32769)}


# A mutant is the model with one rule wrong.  Each must predict, for at least one target of the family it belongs to, another token
# than the oracle emits: a family that no mutant can disturb is not testing its edge.
MUTANT_FAMILY = [("holes_ignored", "filing"), ("skew_ignored", "filing"), ("rewarm_ignored", "filing"), ("rewarm_not_moved", "filing"),
                 ("cut_ignored", "cut"), ("window_32767", "window"), ("window_32769", "window"), ("drop_at_base_plus_1", "trim"),
                 ("skew_at_base_minus_1_dropped", "trim"), ("skew_at_base_without_its_byte", "trim")]


def test_the_mutants_are_the_models():
    assert {m for m, _ in MUTANT_FAMILY} == set(fc.MUTANTS)


@pytest.mark.parametrize("mutant,family", MUTANT_FAMILY, ids=["%s-%s" % (f, m) for m, f in MUTANT_FAMILY])
def test_mutant_of_the_model_is_caught(mutant, family):
    caught = []
    for n in fc.names():
        if fc.family_of(n) != family:
            continue
        c = fc.case(n)
        if not c["targets"]:
            continue
        toks = fc.tokens_at(fc.oracle(c)[0])[0]
        for t in c["targets"]:  # (at the position the prediction is for: p - 1 where the match of p - 1 stays)
            at, tok = fc.predict(c, t, mutant=mutant)[0]
            if tok != toks.get(at):
                caught.append((n, t["p"]))
    print(mutant, len(caught), caught[:6])
    assert caught, "no target of family %s notices: %s" % (family, mutant)


def test_the_model_derives_the_lists_of_every_flush():
    """replay() on a script with every rule in it, against the lists worked out by hand from mi355_deflate_stream_write"""
    calls = fc.replay([2, "F", 1, "F", 29997, "F", 1, 70000, "F", 1, 40000])
    keys = ("lo", "end", "base", "ends", "pts", "skw", "hol", "quirk_end", "e_first", "n_old")
    got = [tuple(s[k] for k in keys) for s in calls]
    assert got[0] == (0, 2, 0, [2], [], [], [], 0, 0, 0)
    # the write of one byte behind the flush at 2: positions 0 and 1 are holes, the re-warm at 2
    assert got[1] == (2, 3, 0, [2, 3], [2], [], [0, 1], 2, 1, 3)
    # the write behind the flush at 3, one byte behind the one at 2: position 1 is re-added, 2 as well, the re-warm moves to 1 and a
    # second one comes at 3 (the write does not fill the input buffer)
    assert got[2] == (3, 30000, 0, [2, 3, 30000], [1, 3], [], [0], 1, 1, 30000)
    # the one-byte write behind 30000: hole at 29999, skew at 30000, re-warm at 30000; three epochs of ident, four in all
    assert got[3] == (30000, 100001, 0, [2, 3, 30000, 100001], [1, 3, 30000], [30000], [0, 29999], 30002, 3, 100001)
    # the flush at 100001 trims to 65536: the lists below it go, the one-byte write behind it adds its own
    assert got[4] == (100001, 140002, 65536, [34465, 74466], [], [100001], [100000], 34467, 3, 74466)
    assert [s["finish"] for s in calls] == [False] * 4 + [True]


def test_flush_diff_names_flush_token_position_epoch_and_lists():
    """what a failing parity test prints"""
    c = fc.case("window_hole_q65535_mod32767_dist32768")
    want = fc.oracle(c)[0]
    assert fc.flush_diff(want, want, c) is None
    got = fc.run_oracle(c["data"], c["opts"], c["plain"])[0]  # (the stream of an encoder that knows no hole)
    msg = fc.flush_diff(got, want, c, flush=1)
    t = c["targets"][0]
    assert t["p"] == 98303
    for part in ("after flush 1", "flush segment 1", "input position 98303 (epoch 2, offset 32767)", "got ('ld', 15, 32768)",
                 "expected ('lit', %d)" % c["data"][98303], "hol [65535]", "skw [65536]", "quirk_end 65538", "e_first 4", "n_old 131330",
                 "target at 98303 (hole, changes, affected position 65535)"):
        assert part in msg, (part, msg)
