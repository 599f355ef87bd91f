"""The hash sort on the GPU (k_sort<0>, k_sort<1>, kb_sort) on the inputs of tests/sort_cases.py: the tables it leaves -- S, the
bucket starts, J, the run flag and the mark -- against the plain reference, exactly, for every case, at every pointer offset the
case lists, with ranks from ballots and from returning LDS atomics; and the bytes of the same calls against the oracle.

The tables are read through mi355_debug_sort_tables, a hook of the test build of the library (`make debug`,
libmi355deflate_dbg.so, tests/dbglib.py).  The test build is a compile of its own: the same source with one dead branch more in
k_sort.  So every case also runs on the product library, alone and all in one batched call, where its stream must equal the
oracle's and inflate to the input.

A sort that mis-ranks is hidden from the stream by design: the walk checks bucket order on the data and the context falls back to
ballot ranks for good.  After all cases with MI355_CFG_SORT_RANKS = 1 the context must still rank from atomics, so no case made
that check fire.  pytest -m gpu."""
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

import dbglib
import oracle_binding as ob
import sort_cases as sc

pytestmark = pytest.mark.gpu

_REF = {}


def oracle(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = ob.encode(c["data"], opts=ob.make_opts(*c["opts"]))
    return _REF[c["name"]]


@pytest.fixture(scope="module")
def dbg():
    """contexts of the test build that rank from ballots (0) and from returning atomics (1; None on a device that failed the order test)"""
    ctxs = {0: dbglib.Ctx(0), 1: dbglib.Ctx(0)}
    ctxs[0].config(3, 0)  # MI355_CFG_SORT_RANKS
    if ctxs[1].sort_ranks() != 1:
        ctxs[1].close()
        ctxs[1] = None
    yield ctxs
    for c in ctxs.values():
        if c:
            c.close()


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


class Placed:
    """a case's bytes in device memory, `off` bytes behind a 16-byte boundary, and an output buffer"""

    def __init__(self, data, off, bound):
        self.n = len(data)
        self.buf = torch.zeros(self.n + 48, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if self.n:
            self.buf[off:off + self.n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        self.cap = bound(self.n) + 16
        self.out = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + off
        torch.cuda.synchronize()

    def stream(self, n):
        return bytes(self.out[:n].cpu().numpy())


def run_on_test_build(cx, c, off):
    """one one-shot device-buffer call of the test build: the stream, and the first difference of its tables from the reference"""
    pl = Placed(c["data"], off, cx.L.mi355_deflate_bound)
    n = cx.encode_device(pl.ptr, pl.n, pl.out.data_ptr(), pl.cap, c["opts"])
    assert cx.passes() == 1, "%s took %d passes: a case must not trigger the first-window re-warm" % (c["name"], cx.passes())
    epochs = (pl.n + sc.EPOCH - 1) // sc.EPOCH
    assert cx.tables_rc(1, epochs) != 0, "the hook handed out an epoch the workspace does not hold"
    S, B = cx.tables(epochs)
    return pl.stream(n), sc.table_diff(c, off, S, B)


@pytest.mark.parametrize("mode", (0, 1), ids=("ballots", "atomics"))
@pytest.mark.parametrize("name", sc.names())
def test_tables_equal_the_reference(dbg, name, mode):
    cx = dbg[mode]
    if cx is None:
        pytest.skip("this device sorts with ballot ranks only")
    c = sc.case(name)
    for off in c["offsets"]:
        got, diff = run_on_test_build(cx, c, off)
        assert diff is None, diff
        assert got == oracle(c), "the test build's stream of %s at offset %d is not the oracle's" % (name, off)
        assert cx.sort_ranks() == mode, "%s at offset %d made the walk's order check fire" % (name, off)


def test_no_case_makes_the_order_check_fire():
    """all cases, at all their offsets, on one fresh context that ranks from atomics: it still does afterwards"""
    cx = dbglib.Ctx(0)
    try:
        started_on_atomics = cx.sort_ranks() == 1
        if started_on_atomics:
            cx.config(3, 1)
        for name in sc.names():
            c = sc.case(name)
            for off in c["offsets"]:
                got, diff = run_on_test_build(cx, c, off)
                assert diff is None, diff
                assert got == oracle(c), (name, off)
        if not started_on_atomics:
            pytest.skip("this device starts on ballot ranks: there is no fallback to watch for")
        assert cx.sort_ranks() == 1, "a case made k_match3's order check fire: the context fell back to ballot ranks"
    finally:
        cx.close()


@pytest.mark.parametrize("name", sc.names())
def test_product_library_gives_the_oracles_bytes(da, ctx, name):
    c = sc.case(name)
    o = da.CompressionOptions(*c["opts"])
    for off in c["offsets"]:
        pl = Placed(c["data"], off, da.bound)
        n = ctx.encode_device(pl.ptr, pl.n, pl.out.data_ptr(), pl.cap, o, compat=1)
        assert ctx.info()["passes"] == 1
        got = pl.stream(n)
        assert got == oracle(c), "%s at offset %d: %d bytes, the oracle %d" % (name, off, len(got), len(oracle(c)))
        assert zlib.decompress(got, -15) == c["data"]


def test_all_cases_in_one_batched_call(da, ctx):
    """kb_sort: every case at every offset it lists, as the items of one encode_batch_device call on the product library"""
    items = [(sc.case(n), off) for n in sc.names() for off in sc.case(n)["offsets"]]
    placed = [Placed(c["data"], off, da.bound) for c, off in items]
    outs, lens, _ = ctx.encode_batch_device([(p.ptr, p.n) for p in placed], [(p.out.data_ptr(), p.cap) for p in placed],
                                            da.CompressionOptions(*sc.DEFAULT), compat=1)
    bi = ctx.batch_info()
    torch.cuda.synchronize()
    assert bi["n_items"] == len(items)
    print("batched:", bi)
    for (c, off), p, n in zip(items, placed, lens):
        got = p.stream(n)
        assert got == oracle(c), "kb_sort on %s at offset %d: %d bytes, the oracle %d" % (c["name"], off, len(got), len(oracle(c)))
        assert zlib.decompress(got, -15) == c["data"]
    empty = sum(1 for c, _ in items if not c["data"])
    # (an item whose speculative parse fails is done again alone, behind the launch set: kb_sort has seen it)
    assert bi["n_batched"] + bi["n_spec_single"] == len(items) - empty and bi["n_q1_single"] == 0, "kb_sort did not see every item (%s)" % (bi,)


def test_alignment_moves_nothing_but_the_run_flag(dbg):
    """the same bytes 0, 1, 8 and 15 bytes behind a 16-byte boundary: identical S, bucket starts and mark; the run flag as the
    reference has it for that alignment (only offset 0 takes the `whole` path and counts run pieces)"""
    cx = dbg[1] or dbg[0]
    for name in ("load_text", "wave_run_33", "hist_even", "natural_rows_96"):
        c = sc.case(name)
        seen = {}
        for off in (0, 1, 8, 15):
            pl = Placed(c["data"], off, cx.L.mi355_deflate_bound)
            n = cx.encode_device(pl.ptr, pl.n, pl.out.data_ptr(), pl.cap, c["opts"])
            assert pl.stream(n) == oracle(c), (name, off)
            epochs = (pl.n + sc.EPOCH - 1) // sc.EPOCH
            S, B = cx.tables(epochs)
            assert sc.table_diff(c, off, S, B) is None, sc.table_diff(c, off, S, B)
            ref = sc.reference(c["data"], off)
            seen[off] = ([S[e][:r["J"]].tobytes() for e, r in enumerate(ref)], [B[e][:sc.EPOCH + 1].tobytes() for e in range(epochs)],
                         [int(B[e][sc.EPOCH + 2]) for e in range(epochs)], [int(B[e][sc.EPOCH + 1]) for e in range(epochs)])
        assert all(seen[off][:3] == seen[0][:3] for off in (1, 8, 15)), name
        assert all(not any(seen[off][3]) for off in (1, 8, 15)), name
    assert seen  # (wave_run_33 and hist_even have the run flag set at offset 0: table_diff held it to the reference)
