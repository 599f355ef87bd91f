"""The permuted-table form of the match walk (k_match3_swz, m3_epoch<.., SWZ = true>: PairWinT<true>, MF_SW1, the five separately
permuted reads of load16) on the inputs of tests/match_cases.py -- every slot of a group, every length and alignment pair of the
16-byte compare, the window and budget edges.

Whether an epoch is walked in that form is k_sort's mark, set from four samples of the sorted array.  The test build of the library
(`make debug`, libmi355deflate_dbg.so, tests/dbglib.py) can force it, mi355_debug_force_swz: 1 = every epoch of 1024 or more
positions is marked (a state that data can produce), 2 = none is; and it reports the marks, mi355_debug_sort_tables.  The test
build is a compile of its own: the same source with one dead branch more in k_sort; the same cases run on the product library in
tests/test_match_walk_gpu.py.

Forms, as there: a case alone is a small call (k_match3_both<.., SINGLE>), a case padded with text to the end of its epoch as
well -- the targets of a case shorter than 1024 positions meet the permuted form that way --, the trains select the both-tables
kernel with whole epochs (the turn-round through the LDS) and in 16 parts without SINGLE, k_match3_swz with whole epochs and in
parts, and a batch is kb_walk.  After every single call the marks are read back: every epoch of 1024 or more positions carries one,
and the targets met in marked epochs are counted against the share tests/test_sort_cases.py works out on the CPU.  Every stream
must equal the oracle's byte for byte, with its block table.

Modes 2 and 0 on the natural inputs of tests/sort_cases.py (rows of records, text): with nothing marked rows go through the plain
table too; with the product's rule the marks read back are the reference's per epoch -- which makes
test_rows_of_records_take_the_permuted_pair_table (tests/test_gpu_parity.py) a test of both forms.  pytest -m gpu."""
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

import dbglib
import match_cases as mc
import oracle_binding as ob
import sort_cases as sc

pytestmark = pytest.mark.gpu

OPTS = sorted({mc.opts_of(n) for n in mc.names()})
PADDED = [n for n in mc.names() if mc.needs_padding(mc.case(n))]
_REF = {}


def oracle(c):
    if c["name"] not in _REF:
        ref = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
        _REF[c["name"]] = (ref, ob.trace_blocks())
    return _REF[c["name"]]


def same_stream(got, c, what):
    ref = oracle(c)[0]
    if got != ref:
        raise AssertionError("%s != oracle (%d vs %d bytes): %s" % (what, len(got), len(ref), mc.match_diff(got, ref, c if "targets" in c else None)))


@pytest.fixture(scope="module")
def cx():
    c = dbglib.Ctx(0)
    c.force_swz(1)
    yield c
    c.close()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def marks(cx, n):
    """(mark, J) per epoch of the last call"""
    ne = (n + mc.EPOCH - 1) // mc.EPOCH
    out = []
    for e0 in range(0, ne, 64):
        _, B = cx.tables(min(64, ne - e0), e0)
        out += [(int(b[mc.EPOCH + 2]), int(b[mc.EPOCH])) for b in B]
    return out


def forced_walk(cx, c, what):
    """one call with the mark forced: the oracle's bytes and block table; returns the number of targets in marked epochs"""
    out = cx.encode(c["data"], c["opts"])
    assert cx.passes() == 1
    bl = cx.blocks()
    same_stream(out, c, what)
    assert bl == oracle(c)[1]
    assert zlib.decompress(out, -15) == c["data"]
    mk = marks(cx, len(c["data"]))
    for e, (m, j) in enumerate(mk):
        assert m == (1 if j >= mc.SWZ_MIN_J else 0), "%s: epoch %d of %d positions has the mark %d" % (what, e, j, m)
    met = [t for t in c["targets"] if mk[t["p"] // mc.EPOCH][0]]
    assert len(met) == len(mc.in_long_epochs(c))
    return len(met)


@pytest.mark.parametrize("name", mc.names())
def test_case_alone(cx, name):
    c = mc.case(name)
    n_ep = (len(c["data"]) + mc.EPOCH - 1) // mc.EPOCH
    assert mc.plan(n_ep, n_cu()) == (16, True, True), "a case alone is no longer a small call's walk"
    forced_walk(cx, c, "the permuted walk of %s alone" % name)


@pytest.mark.parametrize("name", PADDED)
def test_case_padded_to_its_epochs_end(cx, name):
    c = mc.padded(name)
    assert forced_walk(cx, c, "the permuted walk of %s with text behind it" % name) == len(c["targets"])


def test_targets_met_in_marked_epochs(cx):
    """alone or padded, the permuted form meets every target but those of the cases about the end of the input"""
    total = sum(len(mc.case(n)["targets"]) for n in mc.names())
    ends = sum(len(mc.case(n)["targets"]) for n in mc.names() if not mc.in_train(mc.case(n)))
    met = sum(forced_walk(cx, mc.padded(n) if n in PADDED else mc.case(n), n) for n in mc.names())
    print("targets", total, "met in marked epochs", met, "of cases about the end of the input", ends)
    assert met >= total - ends


@pytest.mark.parametrize("level,epochs,lead,want,form", mc.TRAIN_FORMS, ids=["%s_%s_%s" % t[:3] for t in mc.TRAIN_FORMS])
def test_train(cx, level, epochs, lead, want, form):
    tr = mc.train_of(level, epochs, lead)
    n_ep = len(tr["data"]) // mc.EPOCH
    got = mc.plan(n_ep, n_cu())
    assert n_ep == epochs and got == want, "%s: %d epochs on %d compute units give %s, not %s" % (form, n_ep, n_cu(), got, want)
    met = forced_walk(cx, tr, "the permuted walk of %s (%s)" % (tr["name"], form))
    print(tr["name"], "epochs", n_ep, "(split, single, both) =", got, "--", form, "-- targets in marked epochs:", met)
    assert met == len(tr["targets"]) > 0


@pytest.mark.parametrize("opts", OPTS, ids=["%d_%d_%d" % o for o in OPTS])
def test_all_cases_of_a_level_in_one_batch(cx, opts):
    """kb_walk with the mark forced in kb_sort: the cases alone and, where that is short, padded"""
    cs = [mc.case(n) for n in mc.names() if mc.opts_of(n) == opts] + [mc.padded(n) for n in PADDED if mc.opts_of(n) == opts]
    outs = cx.encode_batch([c["data"] for c in cs], opts)
    for k, (c, out) in enumerate(zip(cs, outs)):
        same_stream(out, c, "kb_walk, permuted, on %s (item %d of the batch)" % (c["name"], k))
        assert zlib.decompress(out, -15) == c["data"]


# ---- rows and text with nothing marked, and with the product's rule ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", (2, 0), ids=("none_marked", "product_rule"))
@pytest.mark.parametrize("name", sc.natural_names())
def test_natural_rows(name, mode):
    c = sc.case(name)
    want = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
    cx = dbglib.Ctx(0)
    try:
        cx.force_swz(mode)
        got = cx.encode(c["data"], c["opts"])
        assert cx.passes() == 1
        mk = [m for m, _ in marks(cx, len(c["data"]))]
    finally:
        cx.close()
    ref = [r["mark"] for r in sc.reference(c["data"])]
    assert mk == ([0] * len(ref) if mode == 2 else ref), "%s, mode %d: marks %s, the reference's %s" % (name, mode, mk, ref)
    assert tuple(ref) == sc.NATURAL[c["params"]["natural"]]
    assert got == want, "%s, mode %d: %s" % (name, mode, mc.match_diff(got, want))
    assert zlib.decompress(got, -15) == c["data"]
