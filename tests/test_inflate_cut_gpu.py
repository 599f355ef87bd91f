"""The cuts of a seek handle on the device (include/mi355_deflate.h MI355_CFG_INFLATE_SEEK_CUT_BYTES, mi355_inflate_seek_cuts): for
every case of inflate_cut_cases.py and every cut_bytes the kernels give the cut list, the return value, the count, the report, the
bytes, the untouched fill behind them, the canary and last_read_cuts() that the host build of the same text gives -- the bytes are
zlib's, the cut list is the Python walk's --, alone, in batches and in pieces; damaged streams are rejected as the host build rejects
them; the encoder's own stream reads back with its table and without; and with the key at 0 a handle has no cuts and reads what the
existing path reads.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_cut_cases as cc
import inflcut_binding as cb

pytestmark = pytest.mark.gpu

KEY = ("status", "bit", "out_pos", "out_len", "n_blocks", "n_stored", "n_fixed", "n_dynamic")
FILL, CANARY = cb.FILL, 0xC3


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def key(rep):
    return tuple(rep[k] for k in KEY)


class Arena:
    """a buffer per range in one device tensor: buffer k begins at an 8-byte boundary + k % 8, is filled with FILL and has 64 bytes
    of CANARY behind it"""

    def __init__(self, lens):
        self.lens, self.at, host = list(lens), [], bytearray()
        for k, n in enumerate(self.lens):
            host += bytes(-len(host) % 8 + k % 8)
            self.at.append(len(host))
            host += bytes([FILL]) * n + bytes([CANARY]) * cb.CANARY
        self.t = dev(host + bytes(8))
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.lens[k]]

    def canary_ok(self, k):
        e = self.at[k] + self.lens[k]
        return self.raw[e: e + cb.CANARY] == bytes([CANARY]) * cb.CANARY


class Groups:
    """MI355_CFG_INFLATE_GROUP_BYTES for the calls inside, the default again behind them"""

    def __init__(self, da, ctx, g):
        self.da, self.ctx, self.g = da, ctx, g

    def __enter__(self):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, self.g)
        return self

    def __exit__(self, *exc):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, cb.GROUP_DEFAULT)


def read_batch(ix, s_ptr, ranges):
    """the ranges as one batch on the device: (rc, [(status, got, report key, buffer, canary intact?)])"""
    arena = Arena([ln for _off, ln in ranges])
    rc, res = ix.read_batch_device([(off, ln, arena.ptr(k) if ln else 0) for k, (off, ln) in enumerate(ranges)], s_ptr)
    arena.fetch()
    return rc, [(st, got, key(rep), arena.buf(k), arena.canary_ok(k)) for k, (st, got, rep) in enumerate(res)]


def read_one(ix, s_ptr, off, ln):
    arena = Arena([ln])
    rc, got, rep = ix.read_device(off, ln, arena.ptr(0) if ln else 0, s_ptr)
    arena.fetch()
    return rc, got, key(rep), arena.buf(0), arena.canary_ok(0)


def model(res):
    return [(rc, got, key(rep), buf, canary) for rc, got, rep, buf, canary in res]


@pytest.mark.parametrize("cut", cc.CUT_BYTES)
@pytest.mark.parametrize("name", [c.name for c in cc.corpus()])
def test_every_case_matches_the_host_build(da, ctx, name, cut):
    c = cc.by_name(name)
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, cc.SPACING, c.table, cut=cut)
    host = cb.Index(c.stream, c.wrapper, c.table, cc.SPACING, cut=cut)
    want, _on = cc.cuts(c, cut)
    assert ix.cuts() == host.cuts() == want, (name, cut)
    assert key(ix.report) == key(host.report)
    info = ix.cut_info()
    ends = [b[1] for b in want[1:]] + [len(c.want)]
    assert (info["cut_bytes"], info["n_cuts"]) == (cut, len(want)) and info["host_bytes"] == 24 * len(want) + 8 * (len(c.table) + 1)
    assert info["largest_cut"] == max(e - a[1] for a, e in zip(want, ends))
    ranges = cc.ranges(c, cut, every=False)  # against the host build: every field of every report
    rc, res = read_batch(ix, s.data_ptr(), ranges)
    hrc, hres, hcounts, hcuts = host.read_batch(ranges)
    assert rc == hrc == da.OK and res == model(hres), (name, cut)
    assert ix.last_read() == hcounts and ix.last_read_cuts() == hcuts and hcuts["launches"] == 4
    # EVERY cut boundary - 1 / + 0 / + 1 of the three entries, beginning and ending there, against zlib's slices
    every = cc.ranges(c, cut)
    rc, eres = read_batch(ix, s.data_ptr(), every)
    assert rc == da.OK and ix.last_read_cuts()["launches"] == 4 * ix.last_read()["sets"]
    n = len(c.want)
    for (off, ln), (st, got, k, buf, canary) in zip(every, eres):
        want = c.want[off:off + ln]
        assert st == da.OK and got == len(want) and buf[:got] == want and buf[got:] == bytes([FILL]) * (ln - got) and canary, (name, cut, off, ln)
        assert k[:4] == ("OK", 0, min(off, n) + got, got), (name, cut, off, ln, k)
    for k, (off, ln) in enumerate(ranges):  # one by one: the same
        if k % 9 == 0:
            assert read_one(ix, s.data_ptr(), off, ln) == res[k], (name, cut, off, ln)
            assert ix.last_read_cuts() == host.read(off, ln)[6], (name, cut, off, ln)
    ix.close()


@pytest.mark.parametrize("name", ["text/w0", "fixed/w0", "hand/w0"])
def test_pieces_and_batches_match_the_host_build(da, ctx, name):
    c = cc.by_name(name)
    s = dev(c.stream)
    ranges = [cc.LONG, (0, len(c.want)), (len(c.want) // 2, 70000)]
    with Groups(da, ctx, cb.GROUP_MIN):
        ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=256)
        host = cb.Index(c.stream, 0, c.table, cc.SPACING, cb.GROUP_MIN, 256)
        assert ix.cuts() == host.cuts()  # (the groups of the build do not move the cuts)
        rc, res = read_batch(ix, s.data_ptr(), ranges)
        hrc, hres, hcounts, hcuts = host.read_batch(ranges, group=cb.GROUP_MIN)
        assert rc == hrc == da.OK and res == model(hres) and ix.last_read() == hcounts and ix.last_read_cuts() == hcuts
        assert hcuts["launches"] == 4 * hcounts["sets"]
    for ranges in cc.batches(c, 256):
        rc, res = read_batch(ix, s.data_ptr(), ranges)
        hrc, hres, hcounts, hcuts = host.read_batch(ranges)
        assert rc == hrc == da.OK and res == model(hres) and ix.last_read_cuts() == hcuts and hcounts["sets"] == 1
        for (off, ln), r in zip(ranges, res):
            assert r[3][:r[1]] == c.want[off:off + ln]
    ix.close()


@pytest.mark.parametrize("name", ["text/w0", "hand/w0"])
def test_damaged_streams_are_rejected_as_the_host_build_rejects_them(da, ctx, name):
    """inputs the decoder must reject cleanly: flipped bits in a dynamic header, inside a token, behind the range; zeros for a tail"""
    c = cc.by_name(name)
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=256)
    host = cb.Index(c.stream, 0, c.table, cc.SPACING, cut=256)
    (off, ln), flips, _hdr = cc.damage(c, 256)
    short = c.stream[:len(c.stream) * 3 // 4] + bytes(len(c.stream) - len(c.stream) * 3 // 4)
    failed = 0
    for bad, rng in [(cc.flipped(c.stream, bit), (off, ln)) for _kind, bit in flips] + [(short, (len(c.want) - 5000, 5000)), (short, (10, 100))]:
        d = dev(bad)
        ranges = [rng, (0, 100)]
        rc, res = read_batch(ix, d.data_ptr(), ranges)
        hrc, hres, _counts, hcuts = host.read_batch(ranges, stream=bad)
        assert rc == hrc and res == model(hres) and ix.last_read_cuts() == hcuts, (name, rng)
        failed += rc == da.E_DATA
    assert failed >= 3
    ix.close()


def test_the_encoders_stream_reads_back_with_its_table_and_without(da, ctx):
    data = (cc.vc.pg11() * 2)[1000:201000]
    for wrapper in (0, 2):
        stream = ctx.encode(data, da.CompressionOptions(128, 32, 1), wrapper=wrapper)
        blocks = ctx.blocks()
        ranges = [(0, 100), (len(data) // 2 - 7, 65536), (len(data) - 50, 100), (len(data), 10), (12345, 0)]
        for given in (blocks, None):
            with ctx.inflate_seek(stream, wrapper, cc.SPACING, given, cut=1024) as ix:
                info = ix.cut_info()
                assert info["cut_bytes"] == 1024 and info["n_cuts"] >= len(data) // 2048 and info["largest_cut"] < 1024 + 65536
                assert [ix.read(off, ln) for off, ln in ranges] == [data[off:off + ln] for off, ln in ranges] == ix.read_batch(ranges)
                assert ix.last_read_cuts()["launches"] == 4
    assert ctx.encode(data, da.CompressionOptions(128, 32, 1), wrapper=2) == stream  # the next encode is byte-identical


def test_with_the_key_at_0_a_handle_has_no_cuts(da, ctx):
    """... and reads through the existing path: three launches a set, the existing path's bytes and reports"""
    L = da.load()
    c = cc.by_name("text/w0")
    s = dev(c.stream)
    for value in (63, (1 << 30) + 1):
        assert L.mi355_deflate_ctx_config(ctx._h, 15, value) == da.E_ARG
    ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_BYTES, 4096)  # the key is read at the build ...
    on = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=None)  # (None: the key as the context has it)
    plain = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table)  # cut=0 for the build, 4096 put back behind it
    assert plain.cuts() == [] and ctx.config_get(da.Context.CFG_INFLATE_SEEK_CUT_BYTES) == 4096
    plain.close()
    ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_BYTES, 0)
    off0 = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=None)
    also = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=64)
    assert ctx.config_get(da.Context.CFG_INFLATE_SEEK_CUT_BYTES) == 0
    again = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=None)
    assert on.cut_info()["cut_bytes"] == 4096 and on.cuts() == cc.cuts(c, 4096)[0] and also.cut_info()["cut_bytes"] == 64
    for ix in (off0, again):
        assert ix.cuts() == [] and ix.cut_info() == dict(cut_bytes=0, n_cuts=0, host_bytes=0, largest_cut=0)
    assert on.points() == off0.points() and on.info() == off0.info() and key(on.report) == key(off0.report)
    ranges = cc.ranges(c, 4096)
    rc, res = read_batch(off0, s.data_ptr(), ranges)
    assert off0.last_read_cuts() == dict(cuts=0, symbols=off0.last_read()["symbols"], steps=0, launches=3)
    rc2, res2 = read_batch(on, s.data_ptr(), ranges)
    assert rc == rc2 == da.OK
    for a, b in zip(res, res2):  # the block counts aside, which are those of the cuts decoded
        assert a[:2] == b[:2] and a[2][:4] == b[2][:4] and a[3:] == b[3:]
    n = C.c_size_t(0)
    assert L.mi355_inflate_seek_cuts(on._h, None, 0, C.byref(n)) == da.E_OUT_TOO_SMALL and n.value == len(cc.cuts(c, 4096)[0])
    for ix in (on, off0, also, again):
        ix.close()


def test_the_stage_clocks_time_each_launch_kind_when_asked(da, ctx):
    c = cc.by_name("text/w0")
    s = dev(c.stream)
    on = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table, cut=256)
    off0 = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, cc.SPACING, c.table)
    n = len(c.want)
    assert read_one(on, s.data_ptr(), n - 9000, 5000)[3] == c.want[n - 9000:n - 4000]
    assert ctx.inflate_seek_last_read_stages() == dict(pass1=0, flatten=0, windows=0, resolve=0)  # never, unless asked
    ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
    try:
        assert read_one(on, s.data_ptr(), n - 9000, 5000)[3] == c.want[n - 9000:n - 4000]
        t = ctx.inflate_seek_last_read_stages()
        assert all(v > 0 for v in t.values()), t
        assert read_one(off0, s.data_ptr(), n - 9000, 5000)[3] == c.want[n - 9000:n - 4000]
        t = ctx.inflate_seek_last_read_stages()
        assert t["flatten"] == 0 and t["pass1"] > 0 and t["windows"] > 0 and t["resolve"] > 0, t
    finally:
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
    on.close()
    off0.close()


@pytest.mark.parametrize("name", ["text/w2", "hand/w0"])
def test_the_walker_build_gives_the_same_handle(da, ctx, name):
    """MI355_CFG_INFLATE_SEEK_CUT_WALKER = 1: pass 1 as without cuts, the cuts from a launch that stores no symbol"""
    c = cc.by_name(name)
    s = dev(c.stream)
    a = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, cc.SPACING, c.table, cut=64)
    ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_WALKER, 1)
    try:
        with Groups(da, ctx, cb.GROUP_MIN):
            b = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, cc.SPACING, c.table, cut=64)
    finally:
        ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_WALKER, 0)
    assert b.cuts() == a.cuts() == cc.cuts(c, 64)[0] and b.points() == a.points() and key(b.report) == key(a.report)
    ranges = cc.ranges(c, 64, every=False)
    assert read_batch(b, s.data_ptr(), ranges) == read_batch(a, s.data_ptr(), ranges)
    a.close()
    b.close()
