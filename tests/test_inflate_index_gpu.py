"""The inflate index on the device (include/mi355_deflate.h mi355_inflate_index*, mi355_inflate_parallel*): on every case of
inflate_index_cases.py and at every span size the two kernels leave the candidates and the walkers' records of the host build, and
the table is the host build's; mi355_inflate_parallel_device gives the return value, the report, the bytes and the untouched canary
of the host build, and zlib's bytes; the encoder's own streams come back without their tables at every level and wrapper; groups of
64 KiB; arguments and state.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_index_cases as xc
import inflate_table_cases as tc
import inflindex_binding as xb

pytestmark = pytest.mark.gpu

LV = {"fast": (1, 0, 0), "default": (128, 32, 1), "best": (1768, 128, 1), "rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
KEY = ("status", "bit", "out_pos", "out_len", "n_blocks", "n_stored", "n_fixed", "n_dynamic")
FILL, CANARY = 0xA5, 0xC3


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
    """output buffers of given sizes in one device tensor: buffer k begins at an 8-byte boundary + k % 8, is filled with FILL and
    has 64 bytes of CANARY behind it"""

    def __init__(self, caps):
        self.caps, self.at, host = list(caps), [], bytearray()
        for k, cap in enumerate(self.caps):
            host += bytes(-len(host) % 8 + k % 8)
            self.at.append(len(host))
            host += bytes([FILL]) * cap + bytes([CANARY]) * xb.CANARY
        self.t = dev(host + bytes(8))
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.caps[k]]

    def canary_ok(self, k):
        e = self.at[k] + self.caps[k]
        return self.raw[e: e + xb.CANARY] == bytes([CANARY]) * xb.CANARY


class Setting:
    """a setting of the context for the calls inside, its default again behind them"""

    def __init__(self, ctx, cfg, default):
        self.ctx, self.cfg, self.default, self.now = ctx, cfg, default, default

    def __enter__(self):
        return self

    def set(self, v):
        if v != self.now:
            self.ctx.config(self.cfg, v)
            self.now = v

    def __exit__(self, *exc):
        self.set(self.default)


def spans(da, ctx):
    return Setting(ctx, da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, xb.span_default())


def cap_of(c):
    return len(c.want) if c.want is not None else 1000


@pytest.mark.parametrize("S", [256, 4096, None], ids=["s256", "s4096", "default"])
def test_candidates_records_table_and_bytes_are_the_host_builds(da, ctx, S):
    """per case: the walkers' records (the candidates are their `start`), the table, and through mi355_inflate_parallel_device the return
    code, the report, the bytes, the untouched rest and the canary"""
    S = S or xb.span_default()
    cases = xc.streams()
    arena = Arena([cap_of(c) for c in cases])
    got = []
    with spans(da, ctx) as span:
        span.set(S)
        for k, c in enumerate(cases):
            s = dev(c.stream)
            sp = s.data_ptr() if len(c.stream) else 0
            try:
                table = ctx.inflate_index_device(sp, len(c.stream), c.wrapper)
                rc = da.OK
            except da.DeflateError as e:
                table, rc = None, e.code
            walks = ctx.inflate_index_walks()
            got.append((rc, table, walks, ctx.inflate_device(sp, len(c.stream), arena.ptr(k), cap_of(c), c.wrapper, parallel=True)))
    arena.fetch()
    n_tabled = 0
    for k, c in enumerate(cases):
        rc, table, walks, (prc, pn, prep) = got[k]
        cand, recs = xb.scan(c.stream, c.wrapper, S)
        assert walks == recs and [w[0] for w in walks] == cand, (c.name, S)
        hrc, hn, htable, _chain, _hrep = xb.index(c.stream, c.wrapper, S)
        assert rc == hrc, (c.name, S)
        if rc == da.OK:
            assert [(t["btype"], t["bfinal"], t["n_lz"], t["in_bytes"], t["bit_start"]) for t in table] == \
                   [(t["btype"], t["bfinal"], t["n_tokens"], t["in_bytes"], t["bit_start"]) for t in htable], (c.name, S)
            n_tabled += len(table) >= 2
        want_rc, want_len, want, want_buf, _ = xb.parallel(c.stream, c.wrapper, S, cap_of(c))
        assert (prc, pn, key(prep)) == (want_rc, want_len, key(want)), (c.name, S, prep, want)
        assert arena.buf(k) == want_buf and arena.canary_ok(k), (c.name, S)
        if c.want is not None:
            assert prc == da.OK and arena.buf(k) == c.want, (c.name, S)
        else:
            assert prc == da.E_DATA, (c.name, S)
    assert n_tabled >= 8


def test_damaged_links_and_short_buffers_match_the_host_build(da, ctx):
    c = xc.by_name(xc.MUTATION_BASE)
    _rc, _n, table, _chain, _rep = xb.index(c.stream, 0, 256)
    bits = [t["bit_start"] for t in table] + [8 * len(c.stream)]
    runs = [(m, 600000) for m in xc.mutated([(bits[k], bits[k + 1]) for k in range(len(table))])[::2]]
    z = xc.by_name("zcut/phases")
    _rc, _n, ztable, _chain, _rep = xb.index(z.stream, 0, 256)
    seams = tc.starts([(t["bit_start"], t["in_bytes"]) for t in ztable])
    runs += [(z, cap) for cap in sorted({0, 1, len(z.want) - 1} | {p + d for p in seams[1::3] for d in (-1, 0, 1)})]
    arena = Arena([cap for _m, cap in runs])
    got = []
    with spans(da, ctx) as span:
        span.set(256)
        for k, (m, cap) in enumerate(runs):
            s = dev(m.stream)
            got.append(ctx.inflate_device(s.data_ptr(), len(m.stream), arena.ptr(k) if cap else 0, cap, m.wrapper, parallel=True))
    arena.fetch()
    seen = set()
    for k, (m, cap) in enumerate(runs):
        want_rc, want_len, want, want_buf, _ = xb.parallel(m.stream, m.wrapper, 256, cap)
        rc, n, rep = got[k]
        assert (rc, n, key(rep)) == (want_rc, want_len, key(want)), (m.name, cap, rep, want)
        assert arena.buf(k) == want_buf and arena.canary_ok(k), (m.name, cap)
        if rc == da.OK:
            assert m.want is not None and arena.buf(k)[:n] == m.want, m.name  # never OK with bytes that are not zlib's
        seen.add(rep["status"])
    assert {"OK", "TRUNCATED", "DISTANCE"} <= seen


@pytest.mark.parametrize("level", list(LV))
def test_the_encoders_streams_come_back_without_their_tables(da, ctx, level):
    data = tc.pg11x3()
    for wrapper in (0, 1, 2):
        stream = ctx.encode(data, da.CompressionOptions(*LV[level]), wrapper=wrapper)
        info, blocks = ctx.info(), ctx.blocks()
        s = dev(stream)
        arena = Arena([len(data), len(data)])
        rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), len(data), wrapper, parallel=True)
        rc1, n1, rep1 = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(1), len(data), wrapper)  # one wave
        found = ctx.inflate_index_device(s.data_ptr(), len(stream), wrapper)
        arena.fetch()
        assert (rc, n, rep["status"]) == (da.OK, len(data), "OK"), (level, wrapper, rep)
        assert arena.buf(0) == data and arena.canary_ok(0), (level, wrapper)
        assert (rc1, n1) == (rc, n) and key(rep1) == key(rep) and arena.buf(1) == data and arena.canary_ok(1)
        # the table found is a coarser form of the encoder's: every entry begins where one of the encoder's blocks does
        own = {b["bit_start"]: b for b in blocks}
        assert all(t["bit_start"] in own and t["btype"] == own[t["bit_start"]]["btype"] for t in found)
        assert sum(t["in_bytes"] for t in found) == len(data) and found[-1]["bfinal"] == 1
        assert ctx.verify(stream, data, wrapper, blocks=found)[0] == da.OK  # verify takes it as it stands
        if wrapper == 1:  # host bytes, the size queried first; the one-shot function
            assert ctx.inflate(stream, wrapper, parallel=True) == data
            assert da.inflate_bytes(stream, wrapper, ctx=ctx, parallel=True) == data
            assert ctx.inflate_index(stream, wrapper) == found
        assert ctx.info() == info and ctx.blocks() == blocks  # last_info / last_blocks are the encode's still


def test_several_tabled_groups(da, ctx):
    """MI355_CFG_INFLATE_GROUP_BYTES = 64 KiB: the table of a megabyte of text is worked on in several groups"""
    c = xc.by_name("text/l6")
    s = dev(c.stream)
    arena = Arena([len(c.want)])
    with Setting(ctx, da.Context.CFG_INFLATE_GROUP_BYTES, tc.GROUP_DEFAULT) as groups, spans(da, ctx) as span:
        groups.set(tc.GROUP_MIN)
        span.set(4096)
        table = ctx.inflate_index_device(s.data_ptr(), len(c.stream), 0)
        rc, n, rep = ctx.inflate_device(s.data_ptr(), len(c.stream), arena.ptr(0), len(c.want), 0, parallel=True)
    arena.fetch()
    assert len(table) >= 5 and min(t["in_bytes"] for t in table[:-1]) > tc.GROUP_MIN  # every entry a group of its own
    want = xb.parallel(c.stream, 0, 4096, len(c.want), group=tc.GROUP_MIN)
    assert (rc, n, key(rep)) == (want[0], want[1], key(want[2])) and rc == da.OK
    assert arena.buf(0) == c.want and arena.canary_ok(0)


def test_arguments_state_and_stages(da, ctx):
    L = da.load()
    c = xc.by_name("hand/phases")
    own = da.Context(0)  # (a context of its own: the shard is its state)
    own.config(da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, 256)
    s = dev(c.stream)
    out = torch.empty(len(c.want), dtype=torch.uint8, device="cuda")
    n, r = C.c_size_t(0), da.InflateReport()
    blocks = (da.BlockInfo * 16)()
    for bad in (0, 255, (1 << 30) + 1):
        assert L.mi355_deflate_ctx_config(own._h, da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, bad) == da.E_ARG
    # the room for the table: the query, too small, enough
    assert L.mi355_inflate_index_device(own._h, s.data_ptr(), len(c.stream), 0, None, 0, C.byref(n), C.byref(r), None) == da.E_OUT_TOO_SMALL
    assert n.value == 9
    assert L.mi355_inflate_index_device(own._h, s.data_ptr(), len(c.stream), 0, blocks, 8, C.byref(n), C.byref(r), None) == da.E_OUT_TOO_SMALL
    assert n.value == 9 and blocks[0].in_bytes == 0
    assert L.mi355_inflate_index_device(own._h, s.data_ptr(), len(c.stream), 0, blocks, 9, C.byref(n), C.byref(r), None) == da.OK
    assert n.value == 9 and r.out_len == len(c.want) and [blocks[k].bit_start for k in range(9)] == c.starts
    assert L.mi355_inflate_index_device(own._h, s.data_ptr(), len(c.stream), 3, blocks, 9, C.byref(n), C.byref(r), None) == da.E_ARG
    assert b"bad argument" in L.mi355_deflate_last_error(own._h)
    # a failing chain: MI355_E_DATA, the entries up to and including the failing link
    t = xc.by_name("hand/header_across_the_end")
    ts = dev(t.stream)
    assert L.mi355_inflate_index_device(own._h, ts.data_ptr(), len(t.stream), 0, blocks, 16, C.byref(n), C.byref(r), None) == da.E_DATA
    assert n.value == 3 and da.VERIFY_STATUS[r.status] == "TRUNCATED" and r.out_pos == sum(blocks[k].in_bytes for k in range(3))
    assert b"truncated" in L.mi355_deflate_last_error(own._h)
    # a context that holds a sharded encode refuses, and works again afterwards
    data = tc.pg11x3()[:100000]
    d = dev(data + bytes(64))
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    assert L.mi355_shard_begin(own._h, d.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_inflate_index_device(own._h, s.data_ptr(), len(c.stream), 0, blocks, 16, C.byref(n), C.byref(r), None) == da.E_STATE
        assert L.mi355_inflate_parallel_device(own._h, s.data_ptr(), len(c.stream), 0, out.data_ptr(), len(c.want), C.byref(n), C.byref(r),
                                               None) == da.E_STATE
        assert L.mi355_inflate_parallel(own._h, c.stream, len(c.stream), 0, None, 0, C.byref(n), C.byref(r)) == da.E_STATE
        assert L.mi355_inflate_index(own._h, c.stream, len(c.stream), 0, blocks, 16, C.byref(n), C.byref(r)) == da.E_STATE
    finally:
        L.mi355_shard_end(sh)
    assert L.mi355_inflate_parallel_device(own._h, s.data_ptr(), len(c.stream), 0, out.data_ptr(), len(c.want), C.byref(n), C.byref(r),
                                           None) == da.OK
    assert n.value == len(c.want) and out.cpu().numpy().tobytes() == c.want
    # the stage clocks: no launch times without them, one per launch with them, the same bytes
    ms = own.inflate_index_stages()
    assert ms["find_ms"] == 0 and ms["walk_ms"] == 0 and ms["link_ms"] >= 0
    own.config(da.Context.CFG_STAGE_CLOCKS, 1)
    out.zero_()
    assert own.inflate_device(s.data_ptr(), len(c.stream), out.data_ptr(), len(c.want), 0, parallel=True)[0] == da.OK
    ms = own.inflate_index_stages()
    assert min(ms["find_ms"], ms["walk_ms"]) > 0 and out.cpu().numpy().tobytes() == c.want, ms
    assert own.inflate_tabled_stages()["decode_ms"] > 0
    own.close()
    # the default context (ctx == NULL), host buffers, the size query
    assert L.mi355_inflate_parallel(None, c.stream, len(c.stream), 0, None, 0, C.byref(n), C.byref(r)) == da.E_OUT_TOO_SMALL
    assert n.value == len(c.want)
