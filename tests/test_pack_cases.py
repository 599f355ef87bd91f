"""The inputs of tests/pack_cases.py on the CPU: every case and every train must reach the cells it is there for -- asserted
on a model of the ORACLE's stream alone: block types and phases, stored payload offsets, the first and last bit of every
part and round, long tokens -- and the host build of stages.h (tests/hostsim) must give the oracle's bytes and block table
for it.  With that, a failure of tests/test_pack_gpu.py on the same case points at the parallel code of plan_blocks and
body_k_pack.inc (prefix shortcuts, shared words, the carry between rounds), not at the stage functions.  CPU only."""
import zlib

import pytest

import hostsim_binding as hs
import oracle_binding as ob
import pack_cases as pc

ONE_SHOT = [n for n in pc.names() if "cuts" not in pc._CASES[n]]
HOSTSIM_MAX = 4 << 20


@pytest.mark.parametrize("name", pc.names())
def test_case_reaches_its_cells(name):
    pc.check(pc.case(name))


@pytest.mark.parametrize("name", pc.train_names())
def test_train_members_reach_their_cells_there(name):
    tr = pc.case(name)
    assert len(tr["data"]) >= pc.TRAIN_BLOCKS * pc.B
    got = pc.check_train(tr)
    assert set(got) == set(pc.BODY) | ({name[6:]} if name[6:] else set())


@pytest.mark.parametrize("name", [n for n in ONE_SHOT if n not in ("plain_1024", "plain_1025")] + ["train:", "train:stored_13f", "train:tiny_2_2"])
def test_stage_functions_agree_with_the_oracle(name):
    c = pc.case(name)
    assert len(c["data"]) <= HOSTSIM_MAX
    ref, rb = pc.oracle(c["data"], c["level"])
    rc, out, flags, bl = hs.encode(c["data"], *pc.LV[c["level"]], 1024, 4)
    assert rc == 0 and not (flags & 4)
    assert out == ref, pc.pack_diff(out, ref)
    assert bl == rb
    assert zlib.decompress(ref, -15) == c["data"]


def test_every_cell_of_the_tables_is_reached():
    """the union of all claims: every phase for a group of stored blocks, for a stored block on the serial path and for a
    sync marker; the 16 alignments of a stored payload with both byte values in every shared position; every token-family
    cell, each in a case that runs alone (rounds of 4 096 tokens) and in a train (rounds of 1 024)"""
    claims = {}
    for n in pc.names():
        for x in pc._CASES[n]["claims"]:
            claims.setdefault(x, []).append(n)
    want = [("plain", n) for n in (1, 2, 64, 65, 1024, 1025)]
    want += [("stored_mixed", ph) for ph in range(8)] + [("sync", ph) for ph in range(8)]
    want += [("sync_after", ty) for ty in (0, 1, 2)]
    want += [("stored_align", i, j) for i in range(4) for j in range(4)]
    want += [(k, i, v) for k in ("stored_head", "stored_tail") for i in (1, 2, 3) for v in (0, 255)]
    want += [("stored_final",), ("stored_len", pc.SMALLEST_STORED)] + [("stored_then", ty) for ty in (0, 1, 2)]
    want += [("phase_dep", ty, ph) for ty, ph in ((0, 3), (2, 1), (0, 5), (2, 6), (0, 0))] + [("phase_dep_big", 0), ("phase_dep_big", 2)]
    tokens = [("part_end_aligned", q) for q in (0, 1, 2, 3, "last")] + [("part_start_31",), ("nt0",)]
    tokens += [("round_end_aligned", size) for size in pc.ROUNDS]
    tokens += [("tiny_last_part", k, j) for k in (1, 2, 3) for j in (1, 2, 3)]
    want += tokens + [("long3", w) for w in ("part_first", "wave_last", "round_last", "block_last")]
    want += [("n_enc", n) for n in (256, 257, 258, pc.N_ENC_MAX)] + [("used_hclens", u) for u in pc.USED_HCLENS]
    missing = [x for x in want if x not in claims]
    for ph in range(8):
        if not any(x[0] == "stored_group" and x[1] == ph for x in claims):
            missing.append(("stored_group", ph, "any kind"))
    for kind in ("full", "cnt1", "cnt63", "final_full"):
        if not any(x[0] == "stored_group" and x[2] == kind for x in claims):
            missing.append(("stored_group", "any phase", kind))
    assert not missing, "no case claims %s" % missing
    in_train = set(pc.BODY) | {n[6:] for n in pc.train_names()}
    for x in tokens:
        if x != ("nt0",):  # (an empty block can only end a stream: the trains end with other things)
            assert any(n in in_train for n in claims[x]), "%s is claimed by no member of a train (k_pack<256>)" % (x,)
        assert any(len(pc.case(n)["data"]) <= 64 * pc.B for n in claims[x]), "%s is claimed by no small case (k_pack<1024>)" % (x,)
    assert pc.TOKEN_VARIANTS_SEARCHED == 40 and max(pc.TOKEN_SEEDS) < pc.TOKEN_VARIANTS_SEARCHED


def test_sync_markers_fall_at_every_offset_of_a_word():
    """the marker's 00 00 FF FF is written with one 32-bit put at a byte offset: 0..3 mod 4 all occur, raw or behind the
    two bytes of a zlib header"""
    c = pc.case("sync_phases")
    got = pc.facts(c)
    mod4 = {x[1] for x in got if x[0] == "sync_mod4"}
    assert mod4 | {(m + 2) % 4 for m in mod4} == {0, 1, 2, 3}, mod4
    assert len([x for x in got if x[0] == "sync"]) == 8


def test_the_smallest_stored_block_is_the_smallest():
    """one byte less at the same phase is no longer stored, and the same bytes at phase 0 are not either"""
    front = pc.T(pc.T8[5])
    assert pc.oracle(front + pc.SMALLEST_BYTES, pc.H)[1][1]["btype"] == 0
    assert pc.oracle(front + pc.SMALLEST_BYTES[:-1], pc.H)[1][1]["btype"] != 0
    assert pc.oracle(pc.T(pc.T8[0]) + pc.SMALLEST_BYTES, pc.H)[1][1]["btype"] != 0


def test_the_longest_token_is_what_the_module_records():
    longest = 0
    for name in ("long_round", "long_part", "long_last"):
        c = pc.case(name)
        ms = pc.model(pc.oracle(c["data"], c["level"])[0])
        assert [m["nt"] for m in ms] == [pc.B, pc.LONG_NT]  # (block 1's token indices are what LONG_PLAN says)
        longest = max([longest] + [nb for _, _, nb in ms[1]["long"]])
    assert longest == pc.LONGEST_TOKEN


def test_model_agrees_with_the_block_table():
    """the model is what the claims stand on: its blocks begin where the oracle's table says, its parts and rounds tile the
    block's token bits, and a train's tail read from its first bit gives the blocks the whole stream gives"""
    for name in ("mixed_stored_phases", "tokens_T38", "tiny_3_2", "hdr_284_rle"):
        c = pc.case(name)
        stream, table = pc.oracle(c["data"], c["level"])
        ms = pc.model(stream)
        assert [(m["btype"], m["bfinal"], m["bit_start"]) for m in ms] == [(b["btype"], b["bfinal"], b["bit_start"]) for b in table]
        at = 0
        for m, b in zip(ms, table):
            at += b["in_bytes"]
            if m["btype"] == 0:
                assert m["length"] == b["in_bytes"] and stream[m["ob"]:m["ob"] + m["length"]] == c["data"][at - b["in_bytes"]:at]
                continue
            assert m["nt"] == b["n_lz"]
            assert m["parts"][0][0] == m["bit_start"] + m["hdr_bits"] and m["parts"][-1][1] == m["eob"]
            assert all(a[1] == b2[0] for a, b2 in zip(m["parts"], m["parts"][1:]))
            for size in pc.ROUNDS:
                r = m["rounds"][size]
                assert all(a[3] == b2[2] for a, b2 in zip(r, r[1:])) and (not r or (r[0][2], r[-1][3]) == (m["parts"][0][0], m["eob"]))
    tr = pc.case("train:tiny_1_3")
    stream, table = pc.oracle(tr["data"], tr["level"])
    b0 = tr["members"][-1][1]
    tail = pc.model(stream, table[b0]["bit_start"])
    assert [(m["btype"], m["bit_start"]) for m in tail] == [(b["btype"], b["bit_start"]) for b in table[b0:]]


def test_pack_diff_names_block_part_and_bit():
    """what a failing parity test prints"""
    c = pc.case("tokens_T38")
    want, _ = pc.oracle(c["data"], c["level"])
    assert pc.pack_diff(want, want) is None
    m = pc.model(want)[0]
    bit = m["parts"][2][0] + 5
    got = bytearray(want)
    got[bit >> 3] ^= 1 << (bit & 7)
    msg = pc.pack_diff(bytes(got), want)
    assert msg.startswith("block 0 (type 2") and "part 2 " in msg and "first differing bit %d " % bit in msg, msg
    c = pc.case("stored_13f")
    want, _ = pc.oracle(c["data"], c["level"])
    m = pc.model(want)[1]
    got = bytearray(want)
    got[m["ob"] + m["length"] - 1] ^= 0x80
    msg = pc.pack_diff(bytes(got), want)
    assert msg.startswith("block 1 (type 0") and "tail bytes" in msg, msg
    got = bytearray(want)
    got[m["ob"]] ^= 1
    assert "head bytes" in pc.pack_diff(bytes(got), want)
