"""The inputs and cuts of tests/shard_cases.py on the CPU.  Every case must force what it is there for -- check() asserts its
claims on the model, and that what a rank works out from the bytes it holds is what the whole input gives --, the model's pieces,
the oracle's stream masked to every rank's bit range, must tile that stream, its token counts must add up to the oracle's
tokens, the families must cover the values their names list, and every mutant of the model (one rule of the phases wrong) must
change what the model predicts for at least one case.  With that, a failure of tests/test_shard_gpu.py on a case points at what
only the GPU runs.  The layout of an input too small for ranges of 32 KiB is pinned here too.  CPU only."""
import zlib

import numpy as np
import pytest

import shard_cases as sc

shard = sc.shard


@pytest.mark.parametrize("name", sc.names())
def test_case_forces_what_it_is_there_for(name):
    sc.check(sc.case(name))


@pytest.mark.parametrize("name", sc.names())
def test_model_pieces_tile_the_oracle_stream_and_counts_add_up(name):
    c = sc.case(name)
    m = sc.model_of(c)
    assert sum(m["count"]) == m["T"] == len(m["words"])
    assert sum(len(t) for t in m["tokens"]) == m["T"] and np.array_equal(np.concatenate(m["tokens"]), m["words"])
    if m["ref"] is None:  # (the reference panics: there is no stream)
        assert c["claims"].get("q13_flag") == 2
        return
    assert sc.stitched(c) == m["ref"]
    # the bit ranges are disjoint, in rank order, and cover the stream from its first bit to its last byte
    rs = [b for b in m["bits"] if b is not None]
    assert rs[0][0] == 0 and rs[-1][1] == 8 * len(m["ref"]) and all(x[1] == y[0] for x, y in zip(rs, rs[1:])) and all(x[0] < x[1] for x in rs)
    if not m["hazards"]:
        assert zlib.decompress(m["ref"], -15) == c["data"]


def test_families_cover_the_listed_values():
    cl = {n: sc.case(n)["claims"] for n in sc.names()}
    assert {sc.case(n)["family"] for n in sc.names()} == set(sc.FAMILIES)
    M = lambda n: sc.model_of(sc.case(n))
    off = lambda n, r=1: M(n)["entry"][r] - M(n)["lay"][r]["a"]
    # seam: the range before is left 0 .. 258 and the levels' longest steps into the next one; run-ups that land on, one before and
    # one behind the true entry; ranks whose speculative entry is not the true one
    for lv, longest in (("default", 286), ("best", 382)):
        assert {off(n) for n in sc.names("seam") if n.startswith("seam/seam_%s" % lv)} == set(sc.SEAM_D) | {longest}, lv
    assert all(off(n) < sc.ZONE for n in sc.names("seam"))
    assert [off("seam/runup_default_land%s" % k) for k in ("-1", "0", "+1")] == [0, 0, 1]
    assert sum(1 for n in sc.names("seam") if not all(M(n)["spec_true"])) >= 3
    # count
    assert {M(n)["first"][1] % sc.BLOCK for n in sc.names("count") if "first_mod" in cl[n]} >= {0, 1, sc.BLOCK - 1}
    assert M("count/exact_to_boundary")["nblocks"] == [1, 0, 1] and M("count/exact_to_boundary")["first"][2] == sc.BLOCK
    assert len(M("count/three_fall_short")["pieces"][0]) == 4 and M("count/three_fall_short")["nblocks"][1:4] == [0, 0, 0]
    assert M("count/T_below_a_block")["T"] < sc.BLOCK and M("count/T_below_a_block")["world"] == 8
    assert M("count/T_mod_0")["T"] == sc.BLOCK and M("count/T_mod_0")["count"][1] > 0 and M("count/T_mod_0")["nblocks"] == [1, 1]
    # last
    assert {cl[n]["last_len"] for n in sc.names("last")} == {1, 2, 199, 257}
    m = M("last/empty_final_block_of_an_empty_rank")
    assert m["T"] == sc.BLOCK and m["count"] == [sc.BLOCK, 0] and m["nblocks"] == [1, 1] and m["entry"][1] == 31943 and [b["btype"] for b in m["blocks"]] == [2, 1]
    # short
    assert {s for n in sc.names("short") for s in cl[n]["segs"].values()} == {1, 16, 17, 256, 257}
    assert any(list(cl[n]["segs"].values()) == [1, 1] for n in sc.names("short")) and any(list(cl[n]["segs"].values()) == [1, 1, 1] for n in sc.names("short"))
    assert all(not all(M(n)["spec_true"]) for n in sc.names("short") if "text" not in n)
    # halo
    assert {lo for n in sc.names("halo") for lo in cl[n].get("lo", {}).values()} == {8192, 32768, 33792, 64512}
    assert {k for n in sc.names("halo") for k in cl[n].get("look_ahead", {}).values()} == {1, 257, 258, 259}
    # q13
    assert sorted(cl[n]["q13_flag"] for n in sc.names("q13")) == [1] * 6 + [2]
    assert {tuple(sc.case(n)["cuts"]) for n in sc.names("q13")} == {(0, 66560), (0, 97280), (0, 65536, 98304)}
    b = next(b for b in M("q13/seed1_66560")["blocks"] if b["q13"])
    assert (b["start"], b["start"] + b["in_bytes"]) == (66507, 98328)
    # stored: a rank's first block begins in every quarter of a 32-bit word, on a byte and inside one
    first_bits = [M(n)["bits"][1][0] for n in sc.names("stored")]
    assert {x % 32 // 8 for x in first_bits} == {0, 1, 2, 3} and {x % 8 == 0 for x in first_bits} == {True, False}
    # levels
    assert {sc.case(n)["opts"] for n in sc.names("levels")} == {sc.FAST, sc.GREEDY, sc.RLE, sc.HUFF}


# ---- the layout of a small input ---------------------------------------------------------------------------------------------------------
def test_small_inputs_are_cut_at_multiples_of_1024_or_refused():
    """shard.p1_layout: where the ranks would get less than 32 KiB each, the cuts are multiples of 1024 -- what mi355_shard_begin
    takes --, the layouts cover the input, and an input of fewer than 1024 bytes per rank raises a ValueError that names the limit"""
    for total in (8192, 8193, 100_000, 262_143, 300_000, 5_000_000):
        for world in (1, 2, 3, 8):
            ls = [shard.p1_layout(total, r, world) for r in range(world)]
            assert ls[0]["a"] == 0 and ls[-1]["b"] == total and all(x["b"] == y["a"] for x, y in zip(ls, ls[1:]))
            for L in ls:
                assert L["a"] % 1024 == 0 and L["lo"] % 1024 == 0 and L["a"] < L["b"], (total, world, L)
                assert L["g_lo"] % 32768 == 0 and (L["g_lo"] == 0 or L["g_lo"] <= L["a"] - 32768) and L["g_hi"] == min(total, L["b"] + shard.LOOKAHEAD)
                assert (L["lo"], L["hi"]) == (L["a"] - L["g_lo"], L["b"] - L["g_lo"])
            if total // world >= 32768:  # (unchanged: shard_range's ranges)
                assert [(L["a"], L["b"]) for L in ls] == [shard.shard_range(total, r, world) for r in range(world)]
    assert [shard.p1_layout(8192, r, 8)["a"] for r in range(8)] == [1024 * r for r in range(8)]
    for total, world in ((8191, 8), (1023, 1), (0, 2)):
        with pytest.raises(ValueError, match="1024"):
            shard.p1_layout(total, 0, world)
    assert shard.shard_range(1000, 1, 3) == (333, 666)  # (the chunk-exact path cuts anywhere, as before)


# ---- mutants: the model with one rule wrong ------------------------------------------------------------------------------------------------
def _leave(adv, p, hi):
    while p < hi:
        p += adv[p]
    return p


def _spec_entries(m, w):
    return [_leave(m["adv"], L["a"] - w, L["a"]) if L["a"] >= w else 0 for L in m["lay"]]


def _owners(m, final_to_last):
    first, T = m["first"], m["T"]
    out = []
    for k in range(T // sc.BLOCK + 1):
        t0 = k * sc.BLOCK
        if t0 == T and final_to_last:
            out.append(m["world"] - 1)
        else:  # (the mutant: an empty last block goes to whoever holds the last token)
            out.append(max(r for r in range(m["world"]) if first[r] <= min(t0, T - 1) and m["count"][r]))
    return out


def _q13_flags(m, n):
    out = []
    for k, b in enumerate(m["blocks"]):
        last = k * sc.BLOCK + b["n_lz"] - 1
        full_and_match = b["n_lz"] == sc.BLOCK and int(m["words"][last]) >> 16
        out.append(sc.q13_flag(int(m["tstart"][last]), (int(m["words"][last]) & 0xFF) + 3, True, n) if full_and_match else 0)
    return out


MUTANTS = [
    ("a run-up of 127 positions", lambda m: _spec_entries(m, 127) != m["spec_entry"]),
    ("an entry zone of 382", lambda m: any(382 <= e - L["a"] < sc.ZONE for e, L in zip(m["entry"], m["lay"]))),
    ("a block of 31743 tokens", lambda m: [f % 31743 == 0 for f in m["first"]] != [f % sc.BLOCK == 0 for f in m["first"]]),
    ("an empty last block goes to the last rank with tokens", lambda m: _owners(m, False) != [b["owner"] for b in m["blocks"]]),
    ("Q13 without the end of the input", lambda m: _q13_flags(m, 1 << 40) != [b["q13"] for b in m["blocks"]]),
    ("a rank that is jumped over has tokens", lambda m: any(c == 0 for c in m["count"])),
]


@pytest.mark.parametrize("what,differs", MUTANTS, ids=[x[0].replace(" ", "_") for x in MUTANTS])
def test_mutant_of_the_model_is_caught(what, differs):
    caught = [n for n in sc.names() if differs(sc.model_of(sc.case(n)))]
    print(what, len(caught), caught[:8])
    assert caught, "no case notices: %s" % what
