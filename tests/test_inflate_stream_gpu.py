"""The streaming inflate on the GPU: every case of tests/inflate_stream_cases.py through mi355_inflate_stream_write_device and through
the host form against the host build's model (tests/inflstream) -- return value, bytes handed over, report, state and canary of every
step --, a batch of 70 handles in mixed states in one call, the round trip with the streaming encoder flush by flush, a
MI355_FLUSH_SYNC chunk followed by a FINISH chunk, and the example program's -d --chunk.  The every-byte splits are thinned as the
case module marks them (Script.gpu).  pytest -m gpu."""
import ctypes as C
import io
import os
import random
import subprocess
import sys
import zlib

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_stream_cases as isc
import inflstream_binding as sb
import verify_cases as vc

pytestmark = pytest.mark.gpu
CANARY = sb.CANARY
ROOM = 80000  # the largest cap of a case, and the canary behind it


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    return da.Context(0)


def _rep(r):
    return dict(status=r["status"], bit=r["bit"], out_pos=r["out_pos"], out_len=r["out_len"])


class DeviceHandle:
    """a handle driven through mi355_inflate_stream_write_device, with the model's methods"""

    def __init__(self, ctx, wrapper, zdict, room):
        self.s = ctx.inflate_stream(wrapper, zdict)
        self.room = room  # a device buffer shared by the handles of a test

    def write(self, chunk, cap):
        d_in = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).cuda() if chunk else None
        self.room[cap:cap + CANARY] = 0xC3
        rc, n, rep = self.s.write_device(d_in.data_ptr() if chunk else 0, len(chunk), self.room.data_ptr() if cap else 0, cap)
        assert n <= cap
        back = self.room[:cap + CANARY].cpu().numpy().tobytes() if n else self.room[cap:cap + CANARY].cpu().numpy().tobytes()
        return rc, back[:n] if n else b"", _rep(rep), back[-CANARY:] == b"\xC3" * CANARY

    def finish(self):
        rc, rep = self.s.finish_raw()
        return rc, _rep(rep)

    def state(self):
        return self.s.state()

    def reset(self):
        self.s.reset()

    def close(self):
        self.s.close()


class HostHandle(DeviceHandle):
    """... through mi355_inflate_stream_write on host buffers"""

    def write(self, chunk, cap):
        da = sys.modules["deflate_amd"]
        buf = C.create_string_buffer(b"\xA5" * cap + b"\xC3" * CANARY, cap + CANARY) if cap else None
        n = C.c_size_t(0)
        r = da.InflateReport()
        rc = da.load().mi355_inflate_stream_write(self.s._h, bytes(chunk) if chunk else None, len(chunk), C.cast(buf, C.c_void_p) if cap else None,
                                                  cap, C.byref(n), C.byref(r))
        raw = buf.raw if cap else b""
        assert n.value <= cap
        return rc, raw[:n.value], _rep(r.as_dict()), raw[cap:] == b"\xC3" * CANARY if cap else True


@pytest.fixture(scope="module")
def model_traces():
    """the model's trace of every case that runs on the GPU, computed once"""
    sb.set_mutant(None)
    out = {}
    for s in isc.scripts():
        if not s.gpu:
            continue
        m = sb.Model(s.wrapper, s.zdict)
        out[s.name] = isc.run(m, s)
        m.close()
    return out


@pytest.mark.parametrize("form", ["device", "host"])
def test_every_case_equals_the_host_build(ctx, model_traces, form):
    room = torch.empty(ROOM + CANARY, dtype=torch.uint8, device="cuda")
    cls = DeviceHandle if form == "device" else HostHandle
    n = 0
    for s in isc.scripts():
        if not s.gpu:
            continue
        h = cls(ctx, s.wrapper, s.zdict, room)
        try:
            got = isc.run(h, s)
        finally:
            h.close()
        assert got == model_traces[s.name], (s.name, form, [t[:1] + t[2:4] for t in got if t[0] != "reset"][-3:])
        n += 1
    assert n > 3000


def test_a_batch_of_70_handles_in_mixed_states(da, ctx, model_traces):
    """more handles than lanes, one call: frame pending, mid-stream, done, behind the end, failing, starved for room, one skipped.
    Handle k is driven alone up to step j of its case, step j goes through the batch, the rest alone again: the whole trace must be
    the model's, which is what the same handle driven alone gives (test_every_case_equals_the_host_build)."""
    by = {s.name: s for s in isc.scripts()}
    n_raw = len(isc.bases()[0][1])
    fails = [s.name for s in isc.scripts() if s.name.startswith("fail2+0:")]
    picks = []
    for k in range(14):
        picks += [("prefix:gzip@%d" % (3 + k), 0),                       # the frame header not complete yet
                  ("split2:raw@%d" % (20 + 37 * k % (n_raw - 21)), 1),   # mid-stream
                  ("trailer:after_done:" + ("raw", "zlib", "gzip")[k % 3], 1 + k % 2 * 1),  # done: nothing more (1), a byte behind the end (2)
                  (fails[7 * k % len(fails)], 1),                        # failing
                  (("room:one_less", "room:zero", "room:first_of_two")[k % 3], 0)]  # starved for room
    assert len(picks) == 70
    room = torch.empty(ROOM + CANARY, dtype=torch.uint8, device="cuda")
    hs = [DeviceHandle(ctx, by[name].wrapper, by[name].zdict, room) for name, _ in picks]
    traces = [[] for _ in picks]
    for (name, j), h, t in zip(picks, hs, traces):
        for chunk, cap in by[name].steps[:j]:
            rc, data, rep, ok = h.write(chunk, cap)
            t.append((rc, data, rep, h.state(), ok))
    # the batch: every chunk in one device buffer, every room with its canary in another; item 70 is skipped
    extra = DeviceHandle(ctx, 0, None, room)
    steps = [by[name].steps[j] for name, j in picks] + [(b"\x03\x00", 16)]
    d_in = torch.frombuffer(bytearray(b"".join(c for c, _ in steps)), dtype=torch.uint8).cuda()
    d_out = torch.full((sum(cap + CANARY for _, cap in steps),), 0xC3, dtype=torch.uint8, device="cuda")
    items, a, b = [], 0, 0
    for k, (chunk, cap) in enumerate(steps):
        items.append((d_in.data_ptr() + a if chunk else 0, len(chunk), d_out.data_ptr() + b if cap else 0, cap, da.OK if k < 70 else -99))
        a, b = a + len(chunk), b + cap + CANARY
    rc, reps = ctx.inflate_stream_write_batch_device([h.s for h in hs] + [extra.s], items)
    host = d_out.cpu().numpy().tobytes()
    b, first = 0, da.OK
    for k, (chunk, cap) in enumerate(steps[:70]):
        it = reps.items[k]
        assert it.out_len <= cap
        traces[k].append((it.status, host[b:b + it.out_len], _rep(reps[k]), hs[k].state(), host[b + cap:b + cap + CANARY] == b"\xC3" * CANARY))
        first = first or it.status
        b += cap + CANARY
    assert rc == first != da.OK
    assert reps.items[70].status == -99 and reps.items[70].out_len == 0 and extra.state()["total_in"] == 0
    for (name, j), h, t in zip(picks, hs, traces):
        for chunk, cap in by[name].steps[j + 1:]:
            rc, data, rep, ok = h.write(chunk, cap)
            t.append((rc, data, rep, h.state(), ok))
        rc, rep = h.finish()
        t.append(("finish", rc, rep, h.state()))
        assert t == model_traces[name], (name, j)
        h.close()
    extra.close()
    # handles must be distinct and the context's own
    a, b2 = ctx.inflate_stream(0), ctx.inflate_stream(0)
    other = da.Context(0)
    two = [(0, 0, 0, 0), (0, 0, 0, 0)]
    assert da.load().mi355_inflate_stream_write_batch_device(ctx._h, (C.c_void_p * 2)(a._h, a._h), (da.BatchItem * 2)(), 2, None, None) == da.E_ARG
    assert da.load().mi355_inflate_stream_write_batch_device(other._h, (C.c_void_p * 2)(a._h, b2._h), (da.BatchItem * 2)(), 2, None, None) == da.E_ARG
    assert ctx.inflate_stream_write_batch_device([a, b2], two)[0] == da.OK
    a.close(), b2.close(), other.close()


def test_round_trip_with_the_streaming_encoder_flush_by_flush(da, ctx):
    """what the feature is for: after every flush of a ZlibEncoder the bytes it hands over go into an inflate stream, and the bytes so
    far must be the input so far"""
    rnd = random.Random(20250612)
    text = vc.pg11()
    for case in range(4):
        sizes = [rnd.choice((1, 2, 700, 5000, 31000, 66000)) for _ in range(rnd.randint(3, 6))]
        assert sum(sizes) < 200000
        data = text[case * 1000: case * 1000 + sum(sizes)]
        sink = io.BytesIO()
        enc = da.ZlibEncoder(sink, da.Compression.Default, ctx)
        inf = ctx.inflate_stream(1)
        taken, p, back = 0, 0, b""
        for n in sizes:
            enc.write_all(data[p:p + n])
            p += n
            enc.flush()
            new = sink.getvalue()[taken:]
            taken += len(new)
            assert new.endswith(b"\x00\x00\xff\xff")
            back += inf.write(new)
            assert back == data[:p], (case, sizes, p, len(back))
            assert not inf.done
        new = enc.finish().getvalue()[taken:]
        back += inf.write(new)
        inf.finish()
        st = inf.state()
        assert back == data and st["done"] == 1 and st["adler_or_crc"] == zlib.adler32(data) & 0xFFFFFFFF and st["pending_in"] == 0
        inf.close()


def test_a_sync_chunk_then_a_finish_chunk_as_two_writes(da, ctx):
    data = vc.pg11()[:90000]
    first = ctx.encode(data[:50000], da.Compression.Default, flush=da.FLUSH_SYNC)
    last = ctx.encode(data[50000:], da.Compression.Default, flush=da.FLUSH_FINISH)
    inf = ctx.inflate_stream(0)
    assert inf.write(first) == data[:50000]        # the chunk decodes on its own, all of it
    assert not inf.done and inf.state()["pending_in"] == 0
    assert inf.write(last) == data[50000:]
    assert inf.done
    inf.finish()
    inf.close()


def test_python_batch_and_dictionary(da, ctx):
    zd = vc.pg11()[2000:9000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, zd)
    msgs = [vc.pg11()[3000 + 50 * k: 3400 + 90 * k] for k in range(5)]
    wire = [c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH) for m in msgs]
    a, b = ctx.inflate_stream(0, zd), ctx.inflate_stream(0)
    assert a.write(wire[0]) == msgs[0]
    with pytest.raises(da.DeflateError) as e:
        b.write(wire[0])
    assert e.value.code == da.E_DATA and b.state()["failed"] == "DISTANCE"
    b.reset()
    # many connections, a message each per step
    n = 9
    cs = [zlib.compressobj(6, zlib.DEFLATED, 15) for _ in range(n)]
    hs = [ctx.inflate_stream(1) for _ in range(n)]
    for step in range(3):
        plain = [vc.pg11()[1000 * k + 300 * step: 1000 * k + 300 * step + 100 + 400 * k] for k in range(n)]
        got = ctx.inflate_stream_write_batch(hs, [c2.compress(p) + c2.flush(zlib.Z_SYNC_FLUSH) for c2, p in zip(cs, plain)])
        assert got == plain, step
    for h in hs + [a, b]:
        h.close()


def test_the_example_program_in_chunks(tmp_path):
    exe = str(tmp_path / "cli")
    subprocess.run(["gcc", "-O2", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mi355_deflate_cli.c"),
                    "-L", os.path.join(ROOT, "deflate-rs_amd"), "-lmi355deflate", "-Wl,-rpath," + os.path.join(ROOT, "deflate-rs_amd"), "-o", exe],
                   check=True)
    data = vc.pg11()[:120000]
    for flag, wbits in (("-raw", -15), ("-zlib", 15), ("-gzip", 31)):
        c = zlib.compressobj(6, zlib.DEFLATED, wbits)
        src, whole, pieces = str(tmp_path / "in.bin"), str(tmp_path / "whole.bin"), str(tmp_path / "pieces.bin")
        with open(src, "wb") as f:
            f.write(c.compress(data[:70000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[70000:]) + c.flush())
        subprocess.run([exe, "-d", flag, src, whole], check=True, stderr=subprocess.DEVNULL)
        subprocess.run([exe, "-d", flag, "--chunk", "1000", src, pieces], check=True, stderr=subprocess.DEVNULL)
        assert open(pieces, "rb").read() == open(whole, "rb").read() == data
    bad = str(tmp_path / "bad.bin")
    with open(bad, "wb") as f:
        f.write(zlib.compress(data)[:-1] + b"\0")
    assert subprocess.run([exe, "-d", "-zlib", "--chunk", "1000", bad, str(tmp_path / "x.bin")], stderr=subprocess.DEVNULL).returncode == 3
