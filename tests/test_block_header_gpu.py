"""k_block_header / kb_block_header on the inputs of tests/header_cases.py: histograms that force each of the three length
limiters, numbers of used symbols at the rank sort's chunk edges, ties, and runs of code lengths on the run coder's chunk
seams -- cases the other parity tests' inputs never reach (tests/test_header_cases.py asserts on the CPU that these do, and
that the serial stage functions agree with the oracle on them).  One-input calls and one batch per level, byte for byte
against the oracle; a mismatch is reported by block, tree and symbol.  pytest -m gpu."""
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import header_cases as hc
import oracle_binding as ob

pytestmark = pytest.mark.gpu

LEVELS = sorted({hc.level_of(n) for n in hc.names()})
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


def oracle(name):
    """(stream, block table) of the oracle, made once per case"""
    if name not in _REF:
        _, data, level, _ = hc.case(name)
        ref = ob.encode(data, opts=ob.make_opts(*hc.LV[level]))
        _REF[name] = (ref, ob.trace_blocks())
    return _REF[name]


def same_stream(got, ref, what):
    if got != ref:
        raise AssertionError("%s != oracle (%d vs %d bytes): %s" % (what, len(got), len(ref), hc.header_diff(got, ref)))


@pytest.mark.parametrize("name", hc.names())
def test_one_input_call(da, ctx, name):
    _, data, level, _ = hc.case(name)
    ref, rb = oracle(name)
    out = ctx.encode(data, da.CompressionOptions(*hc.LV[level]), compat=1)
    bl = ctx.blocks()
    same_stream(out, ref, "k_block_header path of %s" % name)
    assert bl == rb
    assert zlib.decompress(out, -15) == data


@pytest.mark.parametrize("level", LEVELS)
def test_all_cases_of_a_level_in_one_batch(da, ctx, level):
    names = [n for n in hc.names() if hc.level_of(n) == level]
    datas = [hc.case(n)[1] for n in names]
    opts = da.CompressionOptions(*hc.LV[level])
    outs = ctx.encode_batch(datas, opts, compat=1)
    bi = ctx.batch_info()
    print(level, bi)
    assert bi["n_items"] == len(names) and bi["n_batched"] + bi["n_single"] == len(names)
    assert bi["n_batched"] == len(names), "an item left the launch set: kb_block_header did not see it"
    for n, d, o in zip(names, datas, outs):
        same_stream(o, oracle(n)[0], "kb_block_header path of %s (item %d of the batch)" % (n, names.index(n)))
        assert o == ctx.encode(d, opts, compat=1), n
        assert zlib.decompress(o, -15) == d
