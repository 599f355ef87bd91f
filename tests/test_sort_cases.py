"""The inputs of tests/sort_cases.py on the CPU.  Every case must reach the cells it claims -- asserted on the reference and on the
restatement of the kernel's pieces, waves and batches alone --, must not send the oracle into a second pass, and a target's match
must be a token of the oracle's; the plain reference must agree with a brute-force sorted() on the small cases; every cell of the
coverage table must be claimed.  Also here, because it is CPU work: the share of the targets of tests/match_cases.py that the
permuted-table walk can meet at all (tests/test_match_walk_swz_gpu.py asserts it on the marks read back).  With that, a failure of
tests/test_sort_gpu.py on a case points at what only the GPU runs.  CPU only."""
import numpy as np
import pytest

import match_cases as mc
import sort_cases as sc


@pytest.mark.parametrize("name", sc.names())
def test_case_reaches_its_cells(name):
    c = sc.case(name)
    assert c["claims"], "a case without a claim"
    sc.check(c)


SMALL = [n for n in sc.names() if not n.startswith("natural_")]


@pytest.mark.parametrize("name", [n for n in SMALL if len(sc.case(n)["data"]) <= 4200] + ["len_32769", "hist_pair", "prev_bucket_32767"])
def test_reference_against_brute_force(name):
    c = sc.case(name)
    ref, bf = sc.reference(c["data"]), sc.brute(c["data"])
    assert len(ref) == len(bf) == (len(c["data"]) + sc.EPOCH - 1) // sc.EPOCH
    for e, (r, (S, B)) in enumerate(zip(ref, bf)):
        assert r["S"].tolist() == S, (name, e)
        assert r["B"].tolist() == B, (name, e)
        assert r["J"] == len(S) == B[-1]


def test_reference_of_the_flags():
    """the run flag and the mark, stated once more by hand on inputs whose answer is plain"""
    z = sc.reference(bytes(sc.EPOCH + 4))
    assert (z[0]["runs"], z[0]["mark"], z[0]["nb"]) == (1, 0, (32, 32, 32, 32)) and z[1]["J"] == 2
    assert sc.reference(bytes(sc.EPOCH + 4), 1)[0]["runs"] == 0 and sc.reference(bytes(sc.EPOCH + 3))[0]["runs"] == 0
    # rows of 256 bytes, every row the same but for a counter: the neighbours of a bucket are 256 bytes apart, on one bank
    rows = sc.reference(sc.records(sc.EPOCH, 256, 1))[0]
    assert rows["mark"] == 1 and min(rows["nb"]) <= 2
    assert sc.reference(sc.records(1025, 256, 1))[0]["mark"] == 0  # (1023 keys)


def test_every_cell_of_the_coverage_table_is_claimed():
    claimed = sc.claimed()
    assert len(set(sc.COVERAGE)) == len(sc.COVERAGE)
    missing = [cell for cell in sc.COVERAGE if cell not in claimed]
    assert not missing, missing
    assert {sc.case(n)["family"] for n in sc.names()} == set(sc.FAMILIES)
    for cell, ns in sorted(claimed.items(), key=repr):
        print(cell, ns)


def test_designed_batches_are_where_the_generator_put_them():
    """the digits written by _low_digits / _high_digits are the digits of the kernel's batches"""
    c = sc.case("hot_low")
    bs = sc.hot_batches(c["data"], 0)["low"]
    h = sc.hashes(c["data"])
    for k, want in enumerate(c["params"]["batches"]):
        at = sc.HOT_LOW_AT + 64 * k
        assert (h[at:at + 64] & 255).tolist() == want and bs[at // 64][1:3] == (want[0], want.count(want[0]))
    c = sc.case("hot_high")
    bs = sc.hot_batches(c["data"], 0)["high"]
    J = len(c["data"]) - 2
    first = (J - J // 3) // 64
    h = sc.hashes(c["data"]).astype(np.int64)
    order1 = np.argsort(h & 255, kind="stable")
    for k, want in enumerate(c["params"]["batches"]):
        keys = order1[64 * (first + k):64 * (first + k + 1)]
        assert set((h[keys] & 255).tolist()) == {255} and (h[keys] >> 8).tolist() == want
        assert bs[first + k][:3] == (64, want[0], want.count(want[0]))
    assert bs[-1][0] == 32 and bs[-1][1:3] == (127, 3)


def test_prev_bucket_targets_are_tokens_of_the_oracle():
    for hv in (sc.EPOCH - 1, 0):
        c = sc.case("prev_bucket_%d" % hv)
        (t,) = c["targets"]
        p, (_, ln, dist) = t["p"], t["tok"]
        assert sc.hash3(*c["data"][p:p + 3]) == hv and p // sc.EPOCH == 1 and (p - dist) // sc.EPOCH == 0
        assert mc.tokens_at(c["data"], c["opts"])[p] == ("ld", ln, dist)
        (length, d), visits = mc.walk(c["data"], p, c["opts"][0])
        assert (length, d) == (ln, dist) and len(visits) == 1, "the bucket holds more than the one candidate"


# ---- the permuted-table walk: how many targets of tests/match_cases.py it can meet -------------------------------------------------------
def test_share_of_match_targets_in_epochs_that_can_be_marked():
    """k_sort marks an epoch only from 1024 positions on.  Alone or padded with text to the end of its last epoch, every case but
    those about the end of the input has all its targets in such epochs; the trains have all of theirs."""
    total = sum(len(mc.case(n)["targets"]) for n in mc.names())
    ends = sum(len(mc.case(n)["targets"]) for n in mc.names() if not mc.in_train(mc.case(n)))
    met = 0
    for n in mc.names():
        c = mc.case(n)
        if mc.needs_padding(c):
            p = mc.padded(n)
            assert len(p["data"]) % mc.EPOCH == 0 and len(mc.in_long_epochs(p)) == len(p["targets"]) == len(c["targets"])
            assert mc.check_train(p) == len(c["targets"])  # (the oracle's tokens at the targets are those of the case alone)
            met += len(p["targets"])
        else:
            met += len(mc.in_long_epochs(c))
            assert not mc.in_train(c) or len(mc.in_long_epochs(c)) == len(c["targets"])
    assert met >= total - ends and ends * 10 < total, (met, total, ends)


@pytest.mark.parametrize("level,epochs,lead", [t[:3] for t in mc.TRAIN_FORMS], ids=["%s_%s_%s" % t[:3] for t in mc.TRAIN_FORMS])
def test_train_targets_lie_in_full_epochs(level, epochs, lead):
    tr = mc.train_of(level, epochs, lead)
    assert len(mc.in_long_epochs(tr)) == len(tr["targets"]) > 0
