"""The tabled inflate on the device (include/mi355_deflate.h mi355_inflate_tabled*): every case of inflate_table_cases.py through
mi355_inflate_tabled_device gets from the three kernels the return value, the report, the bytes and the untouched canary that the host
build of the same three passes gives; the encoder's own streams come back from their block tables at every level and wrapper, in one
group and in groups of 64 KiB, and equal what the one-wave inflate gives; a corrupted trailer is CHECKSUM; a live shard is
MI355_E_STATE; and a tabled call leaves the context's next encode byte-identical.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_table_cases as tc
import infltable_binding as tb

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
            host += bytes([FILL]) * cap + bytes([CANARY]) * tb.CANARY
        self.t = dev(host + bytes(8))
        assert self.t.data_ptr() % 8 == 0
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.caps[k]]

    def canary_ok(self, k):
        e = self.at[k] + self.caps[k]
        return self.raw[e: e + tb.CANARY] == bytes([CANARY]) * tb.CANARY


class Groups:
    """MI355_CFG_INFLATE_GROUP_BYTES for the calls inside, the default again behind them"""

    def __init__(self, da, ctx):
        self.da, self.ctx, self.now = da, ctx, tb.GROUP_DEFAULT

    def __enter__(self):
        return self

    def set(self, g):
        if g != self.now:
            self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, g)
            self.now = g

    def __exit__(self, *exc):
        self.set(tb.GROUP_DEFAULT)


@pytest.mark.parametrize("group", ["oracle", "cut", "wrong", "mutated"])
def test_every_case_matches_the_host_build_of_the_three_passes(da, ctx, group):
    """per call the return code, the report, out[0, out_pos), the untouched rest and the canary are the host build's"""
    runs = [(c, cap) for c, cap in tc.runs() if c.group == group]
    assert len(runs) > 30
    arena = Arena([cap for _c, cap in runs])
    streams = {}
    for c, _cap in runs:
        if c.name not in streams:
            streams[c.name] = dev(c.stream)
    got = []
    with Groups(da, ctx) as groups:
        for k, (c, cap) in enumerate(runs):
            groups.set(c.gbytes)
            s = streams[c.name]
            if tc.refused(c.table):  # MI355_E_ARG from the table's numbers alone
                with pytest.raises(da.DeflateError) as e:
                    ctx.inflate_device(s.data_ptr(), len(c.stream), arena.ptr(k), cap, c.wrapper, blocks=c.table)
                assert e.value.code == da.E_ARG and "bit 0" in str(e.value), (c.name, str(e.value))
                got.append((da.E_ARG, 0, None))
                continue
            got.append(ctx.inflate_device(s.data_ptr() if len(c.stream) else 0, len(c.stream), arena.ptr(k) if cap else 0, cap, c.wrapper,
                                          blocks=c.table))
    arena.fetch()
    n_bad = 0
    for k, (c, cap) in enumerate(runs):
        want_rc, want_len, want, want_buf, _ = tb.inflate(c.stream, c.wrapper, c.table, cap, three=True, group=c.gbytes)
        rc, n, rep = got[k]
        if rep is None:
            assert (want_rc, want_len) == (rc, n) and arena.buf(k) == want_buf == bytes([FILL]) * cap and arena.canary_ok(k), c.name
            continue
        assert (rc, n, key(rep)) == (want_rc, want_len, key(want)), (c.name, cap, rc, rep, want)
        assert arena.buf(k) == want_buf, (c.name, cap)  # the bytes in front of a failure, and FILL from there on
        assert arena.canary_ok(k), (c.name, cap)
        if rc == da.OK:
            assert c.want is not None and arena.buf(k) == c.want, c.name  # never OK with bytes that are not zlib's
        n_bad += rc == da.E_DATA
    if group in ("wrong", "mutated"):
        assert n_bad > 20


@pytest.mark.parametrize("gbytes", [tb.GROUP_DEFAULT, tb.GROUP_MIN])
@pytest.mark.parametrize("level", list(LV))
def test_the_encoders_streams_come_back_from_their_block_tables(da, ctx, level, gbytes):
    data = tc.pg11x3()
    assert 170000 * 2 < len(data) < 600000
    for wrapper in (0, 1, 2):
        stream = ctx.encode(data, da.CompressionOptions(*LV[level]), wrapper=wrapper)
        info, blocks = ctx.info(), ctx.blocks()
        assert len(blocks) >= 3 and sum(b["in_bytes"] for b in blocks) == len(data)
        s = dev(stream)
        arena = Arena([len(data), len(data)])
        with Groups(da, ctx) as groups:
            groups.set(gbytes)
            rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), len(data), wrapper, blocks=blocks)
            if wrapper == 1:  # host bytes, the size queried first; the one-shot function
                assert ctx.inflate(stream, wrapper, blocks=blocks) == data
                assert da.inflate_bytes(stream, wrapper, ctx=ctx, blocks=[(b["bit_start"], b["in_bytes"]) for b in blocks]) == data
        rc1, n1, rep1 = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(1), len(data), wrapper)  # one wave, no table
        arena.fetch()
        assert (rc, n, rep["status"]) == (da.OK, len(data), "OK"), (level, wrapper, rep)
        assert arena.buf(0) == data and arena.canary_ok(0), (level, wrapper)
        assert (rc1, n1) == (rc, n) and key(rep1) == key(rep) and arena.buf(1) == arena.buf(0) and arena.canary_ok(1)
        assert (rep["n_fixed"], rep["n_dynamic"]) == (info["n_fixed"], info["n_dynamic"])
        assert ctx.info() == info and ctx.blocks() == blocks  # last_info / last_blocks are the encode's still


@pytest.mark.parametrize("wrapper", [1, 2])
def test_a_corrupted_trailer_is_checksum(da, ctx, wrapper):
    data = tc.pg11x3()[:200000]
    stream = bytearray(ctx.encode(data, da.Compression.Default, wrapper=wrapper))
    blocks = ctx.blocks()
    stream[-6 if wrapper == 2 else -2] ^= 0x10  # the CRC-32 / the Adler-32
    s = dev(stream)
    arena = Arena([len(data)])
    rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), len(data), wrapper, blocks=blocks)
    arena.fetch()
    assert (rc, n, rep["status"], rep["out_pos"], rep["out_len"]) == (da.E_DATA, len(data), "CHECKSUM", len(data), 0), rep
    assert arena.buf(0) == data and arena.canary_ok(0)
    # ... and is not judged when the buffer is short: the exact size and the prefix
    arena = Arena([1000])
    rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), 1000, wrapper, blocks=blocks)
    arena.fetch()
    assert (rc, n, rep["status"]) == (da.E_OUT_TOO_SMALL, len(data), "OK") and arena.buf(0) == data[:1000] and arena.canary_ok(0)
    with pytest.raises(da.DeflateError) as e:
        ctx.inflate(bytes(stream), wrapper, blocks=blocks)
    assert e.value.code == da.E_DATA


def test_arguments_and_state(da, ctx):
    L = da.load()
    data = tc.pg11x3()[:100000]
    own = da.Context(0)  # (a context of its own: the shard is its state)
    stream = own.encode(data, da.Compression.Default)
    info = own.info()
    arr, nb = own._block_table(own.blocks())
    s = dev(stream)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    n, r = C.c_size_t(0), da.InflateReport()
    args = (s.data_ptr(), len(stream), 0, arr, nb, out.data_ptr(), len(data))
    down = (da.BlockInfo * 2)()
    down[0].bit_start, down[1].bit_start = 8, 0
    late = (da.BlockInfo * 1)()
    late[0].bit_start, late[0].in_bytes = 3, len(data)
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 0, late, 1, out.data_ptr(), len(data), C.byref(n), C.byref(r), None) == da.E_ARG
    assert b"bit 0" in L.mi355_deflate_last_error(own._h)  # the reason of an argument error reaches the caller's context
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 0, down, 2, out.data_ptr(), len(data), C.byref(n), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 3, arr, nb, out.data_ptr(), len(data), C.byref(n), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 0, arr, nb, None, len(data), C.byref(n), C.byref(r), None) == da.E_ARG
    assert L.mi355_deflate_ctx_config(own._h, da.Context.CFG_INFLATE_GROUP_BYTES, tb.GROUP_MIN - 1) == da.E_ARG
    # a context that holds a sharded encode refuses, and works again afterwards
    t = dev(data + bytes(64))
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    assert L.mi355_shard_begin(own._h, t.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_inflate_tabled_device(own._h, *args, C.byref(n), C.byref(r), None) == da.E_STATE
        assert L.mi355_inflate_tabled(own._h, stream, len(stream), 0, arr, nb, None, 0, C.byref(n), C.byref(r)) == da.E_STATE
    finally:
        L.mi355_shard_end(sh)
    assert L.mi355_inflate_tabled_device(own._h, *args, C.byref(n), C.byref(r), None) == da.OK and n.value == len(data)
    assert out.cpu().numpy().tobytes() == data
    # the stage clocks: nothing without them, a time per launch kind with them, the same bytes
    assert own.inflate_tabled_stages() == dict(decode_ms=0, windows_ms=0, resolve_ms=0, checksums_ms=0)
    own.config(da.Context.CFG_STAGE_CLOCKS, 1)
    out.zero_()
    assert L.mi355_inflate_tabled_device(own._h, *args, C.byref(n), C.byref(r), None) == da.OK and out.cpu().numpy().tobytes() == data
    ms = own.inflate_tabled_stages()
    assert min(ms["decode_ms"], ms["windows_ms"], ms["resolve_ms"]) > 0 and ms["checksums_ms"] == 0, ms
    own.config(da.Context.CFG_STAGE_CLOCKS, 0)
    # n_blocks == 0 or no table: the call is the one-wave inflate
    out.zero_()
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 0, arr, 0, out.data_ptr(), len(data), C.byref(n), C.byref(r), None) == da.OK
    assert L.mi355_inflate_tabled_device(own._h, s.data_ptr(), len(stream), 0, None, 0, out.data_ptr(), len(data), C.byref(n), C.byref(r), None) == da.OK
    assert out.cpu().numpy().tobytes() == data and r.n_blocks >= 1
    # a tabled call leaves the context's next encode byte-identical
    assert own.encode(data, da.Compression.Default) == stream and own.info()["out_len"] == info["out_len"]
    own.close()
    # the default context (ctx == NULL)
    assert L.mi355_inflate_tabled_device(None, *args, C.byref(n), C.byref(r), None) == da.OK and n.value == len(data)
