"""The inputs of tests/rewarm_cases.py on the CPU.  Every case must force what it is there for -- asserted on the oracle alone: block
0 holds 31 744 tokens over the bytes the case declares, the predicate restated from lz77.rs:628-638 gives the case's `fires` and w on
the oracle's own tokens, the oracle's token at every target is the model's, and the mutant a target names predicts another one.
Every claim kind has a case, every mutant of the model is caught by some target, and the host build of the stage functions
(stages.h through tests/hostsim) gives the oracle's stream on every case of at most 140 000 bytes.  With that, a failure of
tests/test_rewarm_gpu.py on the same case points at the kernels or the host driver.  CPU only."""
import os
import re

import pytest

import hostsim_binding as hs
import rewarm_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = [n for n in rc.names() if rc.family_of(n) != "paths"]


@pytest.mark.parametrize("name", rc.names())
def test_case_forces_what_it_is_there_for(name):
    c = rc.case(name)
    assert c["family"] == "paths" or len(c["data"]) <= rc.LIMIT
    assert rc.shown(name)


def test_every_claim_kind_has_a_case():
    by = rc.covered()
    assert set(by) == set(rc.names()) and {rc.family_of(n) for n in by} == set(rc.FAMILIES)
    # every edge of the predicate is a pair: one case fires, its twin does not
    got = set().union(*by.values())
    for edge in ("lazy_lit", "lazy_match", "greedy_lit", "greedy_match"):
        assert {edge + "_fires", edge + "_quiet"} <= got, edge
    levels = {rc.opts_of(n) for n in rc.names()}
    assert levels == {rc.DEFAULT, rc.BEST, rc.FAST, rc.GREEDY128, rc.TWO}


@pytest.mark.parametrize("name", SMALL)
def test_host_build_of_the_stages_gives_the_oracles_stream(name):
    c = rc.case(name)
    rcode, out, flags, blocks = hs.encode(c["data"], *c["opts"])
    assert rcode == 0
    assert out == rc.oracle(c), rc.rewarm_diff(out, rc.oracle(c), c)
    assert bool(flags & 1) == c["claims"]["fires"], (name, flags)  # (hostsim.cpp sim_tables: bit 0 = the tables were made a second time)
    assert [(b["n_lz"], b["in_bytes"]) for b in blocks] == [(b["n_lz"], b["in_bytes"]) for b in rc.oracle_blocks(c)]


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_mutant_of_the_model_is_caught(mutant):
    """A mutant is the model with one rule wrong.  Each must predict, for at least one target, another token than the oracle emits."""
    caught = []
    for n in SMALL:
        c = rc.case(n)
        toks = dict(rc.tokens_of(rc.oracle(c)))
        for t in c["targets"]:
            at, tok = rc.predict(c, t, mutant)
            if toks.get(at) != tok:
                caught.append((n, t["p"]))
    print(mutant, len(caught), caught[:6])
    assert caught, "no target notices: %s" % mutant


def test_the_mutants_the_targets_name_are_the_models():
    named = {t["mutant"] for n in rc.names() for t in rc.case(n)["targets"]} - {None}
    assert named == set(rc.MUTANTS), named ^ set(rc.MUTANTS)


def test_the_predicate_on_hand_made_tokens():
    """q1() against lz77.rs:628-638 worked out by hand: the 31 744th token, lazy and greedy, a literal and a match"""
    def toks(tp, tok):
        return [(i, ("lit", 65)) for i in range(rc.BLOCK - 1)] + [(tp, tok)]
    lit, m3 = ("lit", 65), ("ld", 3, 40)
    assert rc.q1(toks(32766, lit), rc.DEFAULT, 50000) == (True, 32768)
    assert rc.q1(toks(32767, lit), rc.DEFAULT, 50000) == (False, 32769)
    assert rc.q1(toks(32765, m3), rc.DEFAULT, 50000) == (True, 32768)
    assert rc.q1(toks(32766, m3), rc.DEFAULT, 50000) == (False, 32769)
    assert rc.q1(toks(32767, lit), rc.GREEDY128, 50000) == (True, 32768)
    assert rc.q1(toks(32768, lit), rc.GREEDY128, 50000) == (False, 32769)
    assert rc.q1(toks(32765, m3), rc.FAST, 50000) == (True, 32768)
    assert rc.q1(toks(32766, m3), rc.FAST, 50000) == (False, 32769)
    tp = rc.BLOCK - 1
    assert [rc.q1(toks(tp, lit), rc.DEFAULT, n)[1] for n in (tp + 1, tp + 2, tp + 3, tp + 4, tp + 5)] == [tp + 1, tp + 1, tp + 1, tp + 2, tp + 2]
    assert rc.q1(toks(tp, lit)[:-1], rc.DEFAULT, 50000) == (False, None)


def test_the_chain_behind_an_identity_entry():
    """chain() on filings worked out by hand from chained_hash_table.rs:64-69,118-158,197-219"""
    import numpy as np
    fh = np.full(4 * rc.W, 7, dtype=np.int64)  # every position in bucket 7 ...
    fh[5000], fh[33000], fh[70000], fh[100000] = 300, 300, 300, 20000  # ... but these
    # epoch 0: bucket 300 is empty in front of 5000, the identity entry is position 300; its own chain is bucket 7 below it,
    # and behind that the identity entry 7 -- which is no lower than the bucket's oldest entry, position 0: the walk ends
    out, hops = rc.chain(fh, 5000)
    assert hops == [300] and out == [300] + list(range(299, -1, -1))
    # epoch 1: 5000 first, then the identity entry behind it
    out, hops = rc.chain(fh, 33000)
    assert out[:2] == [5000, 300] and hops == [300]
    # after the slide: 33000 was filed before it and has lost its successor
    assert rc.chain(fh, 70000) == ([33000], [])
    # a position of epoch 3 with an empty bucket: 65536 + h
    out, hops = rc.chain(fh, 100000)
    assert hops == [65536 + 20000] and out[0] == 65536 + 20000
    assert rc.chain(fh, 100000, "no_hops") == ([], []) and rc.chain(fh, 100000, "hops_two_epochs") == ([], [])
    assert rc.chain(fh, 33000, "hops_two_epochs")[1] == [300]
    assert [rc.base_of(p) for p in (0, 65535, 65536, 98303, 98304)] == [0, 0, 32768, 32768, 65536]


def test_the_streamed_case_is_the_smallest_that_takes_the_streamed_host_call():
    src = open(os.path.join(HERE, "..", "deflate-rs_amd", "csrc", "deflate_host.inc")).read()
    m = re.search(r"constexpr size_t HOST_PIECEWISE_FROM = (\d+)u << (\d+);", src)
    assert m and int(m.group(1)) << int(m.group(2)) == rc.HOST_PIECEWISE_FROM
    assert "in_len >= HOST_PIECEWISE_FROM" in src
    m = re.search(r"#define MI355_IDENT_EPOCHS (\d+)", src)
    assert m and int(m.group(1)) == rc.IDENT_EPOCHS
    assert len(rc.case("paths_default_hop_streamed")["data"]) == rc.HOST_PIECEWISE_FROM


def test_rewarm_diff_names_token_position_epoch_w_and_chain():
    """what a failing parity test prints"""
    import oracle_binding as ob
    c = rc.case("hop_default_after_slide_w32768")
    want = rc.oracle(c)
    assert rc.rewarm_diff(want, want, c) is None
    other = bytearray(c["data"])
    other[65536] ^= 0x15  # (the stream of an input without the copy: literals where the hop found the match)
    got = ob.encode(bytes(other), opts=ob.make_opts(*c["opts"]))
    msg = rc.rewarm_diff(got, want, c)
    for part in ("input position 65536 (epoch 2, offset 0)", "expected ('ld', 9, 32768)", "w 32768 (fires)", "32768*=9",
                 "target at 65536 (hop_after_slide, mutant no_hops)"):
        assert part in msg, (part, msg)
