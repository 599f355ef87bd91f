"""The inputs of tests/header_cases.py on the CPU: every case must provoke what it is there for -- asserted on the oracle
alone: block type, depth of the unlimited Huffman tree, number of used symbols, runs of equal code lengths with their first
and last entry -- and the host build of stages.h (tests/hostsim) must give the oracle's bytes and block table for it.  With
that, a failure of tests/test_block_header_gpu.py on the same case points at the wave-parallel code of k_block_header
(wave_huff, the run coder by ballots), not at the stage functions.  CPU only."""
import zlib

import pytest

import header_cases as hc
import hostsim_binding as hs
import oracle_binding as ob


@pytest.mark.parametrize("name", hc.names())
def test_case_provokes_what_it_is_there_for(name):
    hc.check(hc.case(name))


@pytest.mark.parametrize("name", hc.names())
def test_stage_functions_agree_with_the_oracle(name):
    _, data, level, _ = hc.case(name)
    c, l, m = hc.LV[level]
    ref = ob.encode(data, opts=ob.make_opts(c, l, m))
    rb = ob.trace_blocks()
    rc, out, flags, bl = hs.encode(data, c, l, m, 1024, 4)
    assert rc == 0 and not (flags & 4)
    assert out == ref, hc.header_diff(out, ref)
    assert bl == rb
    assert zlib.decompress(ref, -15) == data


def test_every_limiter_and_every_chunk_count_is_reached():
    """the table as a whole: trees over each of the three limits and exactly at them, every number of keys a lane of the
    rank sort can hold, distance trees of 0, 1, 2 and 30 codes"""
    blocks = [b for n in hc.names() for b in hc.case(n)[3]]
    for key, limit, over in (("ll_unl", 15, {16, 17, 20}), ("d_unl", 15, {16, 17, 18}), ("cl_unl", 7, {8, 9})):
        seen = {b[key] for b in blocks if key in b}
        assert limit in seen and over <= seen, (key, sorted(seen))
    assert {(b["m_ll"] + 63) // 64 for b in blocks if "m_ll" in b} == {1, 2, 3, 4, 5}
    assert {b["m_ll"] for b in blocks if "m_ll" in b} >= {2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 286}
    assert {b["m_d"] for b in blocks if "m_d" in b} >= {0, 1, 2, 30}
    runs = [r for b in blocks for r in b.get("runs", ())]
    assert {e - s for s, e, v in runs if v == 0} >= {1, 2, 3, 10, 11, 138, 139, 140, 141, 149, 190, 255}
    assert {e - s for s, e, v in runs if v} >= {3, 4, 6, 7, 8, 128}
    assert {s for s, e, v in runs} >= {64, 128, 192} and {e for s, e, v in runs} >= {64, 128, 192}
    assert any(s < 64 and e > 192 for s, e, v in runs) and any(s < 256 < e for s, e, v in runs)
    assert sum(1 for b in blocks if b.get("seam")) >= 4


def test_decoder_reads_back_the_input():
    """the inflate of header_cases.py is what the preconditions stand on: its tokens give the input back, at a level with
    matches and over several blocks"""
    for name in ("a_three_blocks", "b_dist17_default", "d_m286", "e_seam_runs_rle"):
        _, data, level, _ = hc.case(name)
        stream = ob.encode(data, opts=ob.make_opts(*hc.LV[level]))
        blocks = hc.decode(stream)
        assert hc.inflate(blocks) == data
        assert [b["bit_start"] for b in blocks] == [b["bit_start"] for b in ob.trace_blocks()]
        assert hc.header_diff(stream, stream) is None


def test_header_diff_names_block_tree_and_symbol():
    """what a failing parity test prints: the first block, the tree and the first symbol whose lengths differ"""
    _, data, level, _ = hc.case("a_three_blocks")
    want = ob.encode(data, opts=ob.make_opts(*hc.LV[level]))
    # the second block's bytes with two values swapped: its literal/length lengths change, the first block's do not
    second = data[hc.BLOCK_TOKENS:2 * hc.BLOCK_TOKENS]
    vals = sorted(set(second), key=second.count)
    a, b = vals[0], vals[-1]
    swapped = second.translate(bytes(b if v == a else a if v == b else v for v in range(256)))
    got = ob.encode(data[:hc.BLOCK_TOKENS] + swapped + data[2 * hc.BLOCK_TOKENS:], opts=ob.make_opts(*hc.LV[level]))
    msg = hc.header_diff(got, want)
    ll_want = hc.decode(want)[1]["ll_lens"]
    assert msg.startswith("block 1 (bit %d), literal/length tree: symbol %d has length " % (hc.decode(want)[1]["bit_start"], min(a, b)))
    assert msg.endswith("expected %d" % ll_want[min(a, b)])
    # a stream cut short is reported, not raised
    assert "block 2" in hc.header_diff(want[:len(want) // 2 + 9000], want) or "block 1" in hc.header_diff(want[:len(want) // 2 + 9000], want)
