"""The inflate entry points on the device (include/mi355_deflate.h mi355_inflate*): every case of inflate_cases.py through the
batch entry gets from k_inflate the report and the bytes the host build of the same decisions gives, and zlib's bytes where zlib
accepts the stream; the encoder's packed arenas inflate back to their inputs at every level and wrapper; a failing or short item
disturbs no neighbour; the size query, the skip rule and the argument and state errors.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_cases as icase
import inflwrite_binding as iw
import verify_cases as vc

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
    """output buffers of given sizes in one device tensor: buffer k begins at an 8-byte boundary + k % 4, is filled with FILL and
    has 64 bytes of CANARY behind it"""

    def __init__(self, caps):
        self.caps, self.at, host = list(caps), [], bytearray()
        for k, cap in enumerate(self.caps):
            host += bytes(-len(host) % 8 + k % 4)
            self.at.append(len(host))
            host += bytes([FILL]) * cap + bytes([CANARY]) * iw.CANARY
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
        return self.raw[e: e + iw.CANARY] == bytes([CANARY]) * iw.CANARY


@pytest.mark.parametrize("wrapper", [0, 1, 2])
def test_corpus_through_the_batch_entry_matches_the_host_build_and_zlib(da, ctx, wrapper):
    """one batch per wrapper; per item the return code, the report, out[0, out_pos) and the untouched rest are the host build's"""
    cases = [c for c in icase.corpus() if c.wrapper == wrapper]
    assert len(cases) > (600 if wrapper < 2 else 20)
    caps = [iw.cap_for(c.stream, c.wrapper, c.want) for c in cases]
    arena = Arena(caps)
    blob = dev(b"".join(c.stream for c in cases))
    items, at = [], 0
    for k, c in enumerate(cases):
        items.append((blob.data_ptr() + at, len(c.stream), arena.ptr(k) if caps[k] else 0, caps[k]))
        at += len(c.stream)
    rc, reps = ctx.inflate_batch_device(items, wrapper)
    arena.fetch()
    first = da.OK
    n_bad = 0
    for k, (c, rep) in enumerate(zip(cases, reps)):
        want_rc, want_len, want, want_buf, _ = iw.inflate(c.stream, c.wrapper, caps[k], lanes=True)
        it = reps.items[k]
        assert (it.status, it.out_len) == (want_rc, want_len) and key(rep) == key(want), (c.name, it.status, rep, want)
        assert arena.buf(k) == want_buf, c.name  # the bytes in front of a failure, and FILL from there on
        assert arena.canary_ok(k), c.name
        if c.want is not None:
            assert it.status == da.OK and arena.buf(k) == c.want, c.name
        else:
            assert it.status == da.E_DATA, (c.name, rep)
            n_bad += 1
        if first == da.OK:
            first = it.status
    assert rc == first and n_bad > 5


ROUND_TRIP = None


def round_trip_items():
    global ROUND_TRIP
    if ROUND_TRIP is None:
        text = vc.pg11()
        ROUND_TRIP = [b"", b"Q", text[5000:5000 + 4096], (text * 2)[1000:1000 + 65536], vc.noise(32768, 7), text]
    return ROUND_TRIP


@pytest.mark.parametrize("level", list(LV))
def test_packed_arenas_inflate_back_to_their_inputs(da, ctx, level):
    datas = round_trip_items()
    ins = [dev(d) for d in datas]
    for wrapper in (0, 1, 2):
        res = ctx.encode_batch_packed_device(ins, None, da.CompressionOptions(*LV[level]), wrapper=wrapper)
        info = ctx.info()
        arena = Arena([len(d) for d in datas])
        base = res.arena.data_ptr()
        items = [(base + off, n, arena.ptr(k) if datas[k] else 0, len(datas[k])) for k, (off, n) in enumerate(res.entries)]
        rc, reps = ctx.inflate_batch_device(items, wrapper)
        assert rc == da.OK, reps
        arena.fetch()
        for k, d in enumerate(datas):
            assert reps[k]["status"] == "OK" and reps.items[k].out_len == len(d), (level, wrapper, k, reps[k])
            assert arena.buf(k) == d and arena.canary_ok(k), (level, wrapper, k)
        assert ctx.info() == info  # an inflate leaves the encode's records alone


@pytest.mark.parametrize("wrapper", [0, 1, 2])
def test_single_stream_calls(da, ctx, wrapper):
    data = vc.pg11()
    stream = ctx.encode(data, da.Compression.Default, wrapper=wrapper)
    info, blocks = ctx.info(), ctx.blocks()
    assert zlib.decompressobj(vc.WBITS[wrapper]).decompress(stream) == data
    s = dev(stream)
    arena = Arena([len(data)])
    rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), len(data), wrapper)
    arena.fetch()
    assert (rc, n, rep["status"], rep["out_pos"]) == (da.OK, len(data), "OK", len(data)), rep
    assert arena.buf(0) == data and arena.canary_ok(0)
    assert (rep["n_fixed"], rep["n_dynamic"]) == (info["n_fixed"], info["n_dynamic"])
    assert ctx.inflate(stream, wrapper) == data  # host bytes, the size queried first
    assert da.inflate_bytes(stream, wrapper, ctx=ctx) == data
    assert ctx.info() == info and ctx.blocks() == blocks  # last_info / last_blocks are the encode's still
    # the size query: no buffer at all
    rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), 0, 0, wrapper)
    assert (rc, n, rep["status"], rep["out_len"]) == (da.E_OUT_TOO_SMALL, len(data), "OK", len(data)), rep
    # a short buffer: the prefix, the exact size, nothing behind it
    arena = Arena([1000])
    rc, n, rep = ctx.inflate_device(s.data_ptr(), len(stream), arena.ptr(0), 1000, wrapper)
    arena.fetch()
    assert (rc, n) == (da.E_OUT_TOO_SMALL, len(data)) and arena.buf(0) == data[:1000] and arena.canary_ok(0)
    # a damaged stream through both single entries: the host build's report
    bad = stream[:len(stream) // 2]
    cap = iw.cap_for(bad, wrapper, None)
    want_rc, want_len, want, want_buf, _ = iw.inflate(bad, wrapper, cap, lanes=True)
    assert want_rc == da.E_DATA
    rc, n, rep, held = ctx.inflate_raw(bad, wrapper, cap)
    assert (rc, n, key(rep)) == (want_rc, want_len, key(want)) and held == want_buf[:want_len], (rep, want)
    with pytest.raises(da.DeflateError) as e:
        ctx.inflate(bad, wrapper)
    assert e.value.code == da.E_DATA


def test_a_failing_or_short_item_disturbs_no_neighbour(da, ctx):
    text = vc.pg11()
    datas = [text[2500 * k: 2500 * k + 2000 + 37 * k] for k in range(64)]
    streams = [zlib.compress(d, 6) for d in datas]
    streams[5] = streams[5][:-2] + bytes([streams[5][-2] ^ 0x40]) + streams[5][-1:]  # the Adler-32
    streams[20] = streams[20][:-9]
    streams[41] = streams[41][:300] + bytes([streams[41][300] ^ 0x04]) + streams[41][301:]
    caps = [len(d) for d in datas]
    caps[9] -= 1
    caps[50] = 0
    arena = Arena(caps)
    blob = dev(b"".join(streams))
    items, at = [], 0
    for k, s in enumerate(streams):
        items.append((blob.data_ptr() + at, len(s), arena.ptr(k) if caps[k] else 0, caps[k]))
        at += len(s)
    rc, reps = ctx.inflate_batch_device(items, 1)
    arena.fetch()
    assert rc == da.E_DATA  # item 5 is the first that fails
    for k in range(64):
        it = reps.items[k]
        assert arena.canary_ok(k), k
        if k in (5, 20, 41):
            want_rc, want_len, want, want_buf, _ = iw.inflate(streams[k], 1, caps[k], lanes=True)
            assert want_rc == da.E_DATA and (it.status, it.out_len, key(reps[k])) == (want_rc, want_len, key(want)), (k, reps[k], want)
            assert arena.buf(k) == want_buf, k
        elif k in (9, 50):
            assert (it.status, it.out_len, reps[k]["status"]) == (da.E_OUT_TOO_SMALL, len(datas[k]), "OK"), (k, reps[k])
            assert arena.buf(k) == datas[k][:caps[k]], k
        else:
            assert (it.status, it.out_len, reps[k]["status"]) == (da.OK, len(datas[k]), "OK"), (k, reps[k])
            assert arena.buf(k) == datas[k], k
    assert reps[5]["status"] == "CHECKSUM" and reps[20]["status"] == "TRUNCATED"


def test_items_with_a_status_on_entry_are_skipped(da, ctx):
    data = vc.pg11()[:3000]
    stream = dev(zlib.compress(data, 6)[2:-4])
    arena = Arena([3000, 3000, 3000])
    items = (da.BatchItem * 3)()
    for k in range(3):
        items[k].in_, items[k].in_len, items[k].out, items[k].out_cap = stream.data_ptr(), stream.numel(), arena.ptr(k), 3000
        items[k].out_len = 77
    items[1].status = da.E_UNSUPPORTED
    reps = (da.InflateReport * 3)()
    C.memset(reps, 0xEE, C.sizeof(reps))
    rc = da.load().mi355_inflate_batch_device(ctx._h, items, 3, 0, reps, None)
    arena.fetch()
    assert rc == da.OK and [items[k].status for k in range(3)] == [da.OK, da.E_UNSUPPORTED, da.OK]
    assert [items[k].out_len for k in range(3)] == [3000, 77, 3000]
    assert arena.buf(0) == data and arena.buf(2) == data and arena.buf(1) == bytes([FILL]) * 3000
    assert bytes(reps[1]) == b"\xEE" * C.sizeof(da.InflateReport) and reps[0].status == 0 and reps[2].out_len == 3000
    # every item skipped, and no item at all: nothing to do
    items[0].status = items[2].status = da.E_DATA
    assert da.load().mi355_inflate_batch_device(ctx._h, items, 3, 0, None, None) == da.OK
    assert da.load().mi355_inflate_batch_device(ctx._h, None, 0, 0, None, None) == da.OK


def test_arguments_and_state(da, ctx):
    L = da.load()
    data = vc.pg11()
    stream = ctx.encode(data, da.Compression.Default)
    info = ctx.info()
    s = dev(stream)
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    n, r = C.c_size_t(0), da.InflateReport()
    args = (s.data_ptr(), len(stream), 0, out.data_ptr(), len(data))
    for bad in ((s.data_ptr(), len(stream), 3, out.data_ptr(), len(data)), (s.data_ptr(), len(stream), -1, out.data_ptr(), len(data)),
                (0, len(stream), 0, out.data_ptr(), len(data)), (s.data_ptr(), len(stream), 0, 0, len(data))):
        assert L.mi355_inflate_device(ctx._h, bad[0], bad[1], bad[2], bad[3], bad[4], C.byref(n), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_device(ctx._h, *args, None, C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_device(ctx._h, *args, C.byref(n), None, None) == da.E_ARG
    assert L.mi355_inflate(ctx._h, stream, len(stream), 0, None, 10, C.byref(n), C.byref(r)) == da.E_ARG
    assert L.mi355_inflate(ctx._h, None, 10, 0, None, 0, C.byref(n), C.byref(r)) == da.E_ARG
    with pytest.raises(da.DeflateError) as e:
        ctx.inflate_batch_device([(s.data_ptr(), len(stream), out.data_ptr(), len(data))], 3)
    assert e.value.code == da.E_ARG
    with pytest.raises(da.DeflateError) as e:
        ctx.inflate_batch_device([(s.data_ptr(), len(stream), 0, len(data))], 0)  # a size without a buffer
    assert e.value.code == da.E_ARG
    assert L.mi355_inflate_batch_device(ctx._h, None, 2, 0, None, None) == da.E_ARG
    # a context that holds a sharded encode refuses, and works again afterwards (a context of its own: the shard is its state)
    own = da.Context(0)
    keep, ctx = ctx, own
    t = dev(data + bytes(64))
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    assert L.mi355_shard_begin(ctx._h, t.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_inflate_device(ctx._h, *args, C.byref(n), C.byref(r), None) == da.E_STATE
        assert L.mi355_inflate(ctx._h, stream, len(stream), 0, None, 0, C.byref(n), C.byref(r)) == da.E_STATE
        with pytest.raises(da.DeflateError) as e:
            ctx.inflate_batch_device([(s.data_ptr(), len(stream), out.data_ptr(), len(data))], 0)
        assert e.value.code == da.E_STATE
    finally:
        L.mi355_shard_end(sh)
    assert L.mi355_inflate_device(ctx._h, *args, C.byref(n), C.byref(r), None) == da.OK and n.value == len(data)
    assert out.cpu().numpy().tobytes() == data
    own.close()
    ctx = keep
    # the default context (ctx == NULL)
    assert L.mi355_inflate_device(None, *args, C.byref(n), C.byref(r), None) == da.OK and n.value == len(data)
    assert stream == ctx.encode(data, da.Compression.Default) and ctx.info()["out_len"] == info["out_len"]
