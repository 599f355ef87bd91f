"""The checksum kernels on the device (k_adler_part / k_adler_fold, k_crc_part / k_crc_fold, kb_adler_part, kb_crc) over the cases
of tests/checksum_cases.py: the two single entries on every case against zlib; the batched kernels with chosen bytes through
verify_batch_device, and over unaligned outputs through inflate_batch_device and inflate_device; the trailers the batched
encodes write; one case past 2^31 bytes.  tests/test_checksum_cases.py holds the same lists to a model of the kernels on the CPU.
Needs a real MI355X: pytest -m gpu."""
import functools
import os
import struct
import sys
import time
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import checksum_cases as cc

pytestmark = pytest.mark.gpu

WBITS = {1: 15, 2: 31}
FILL, CANARY = 0xA5, 0xC3
OUT_OFFSETS = (0, 1, 3, 4, 8, 15)


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


def upload(buf):
    t = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    assert t.data_ptr() % 32 == 0  # (what the cases' offsets are counted from)
    return t


def dev(b):
    return torch.frombuffer(bytearray(bytes(b) + bytes(8)), dtype=torch.uint8).cuda()


# ---- the single entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
@pytest.mark.parametrize("kind", ("adler", "crc"))
def test_single_entry_on_every_case(da, ctx, kind, family):
    """sizes x details x offsets of one family from one arena, uploaded once; the guard bytes around a case are not zero, so a read
    past either end of it changes the sum"""
    buf, cases = cc.arena(kind, family)
    t = upload(buf)
    fn = ctx.adler32_device if kind == "adler" else ctx.crc32_device
    bad = []
    for c in cases:
        got, want = fn(t.data_ptr() + c.at, c.n), cc.reference(kind, cc.case_bytes(buf, c))
        if got != want:
            bad.append("%s: %08x, zlib %08x" % (cc.case_id(c), got, want))
    assert not bad, "%d of %d cases: %s" % (len(bad), len(cases), "; ".join(bad[:8]))


def test_a_call_leaves_nothing_behind(da):
    ctx = da.Context(0)  # (its own: the order of the calls is the test)
    try:
        buf, cases = cc.build_arena([("random", None, 393217, 1), ("ff", None, 147428, 0)])
        t = upload(buf)
        big, ff = cases
        want = {k: [cc.reference(k, cc.case_bytes(buf, c)) for c in cases] for k in ("adler", "crc")}
        # a call of size 0 behind a large one
        assert ctx.crc32_device(t.data_ptr() + big.at, big.n) == want["crc"][0]
        assert ctx.crc32_device(t.data_ptr() + big.at, 0) == 0 and ctx.crc32_device(0, 0) == 0
        assert ctx.adler32_device(t.data_ptr() + big.at, big.n) == want["adler"][0]
        assert ctx.adler32_device(t.data_ptr() + big.at, 0) == 1 and ctx.adler32_device(0, 0) == 1
        # a large call behind an encode, whose records stay
        data = cc.case_bytes(buf, ff) + cc.case_bytes(buf, big)[:70000]
        for wrapper in (1, 2):
            stream = ctx.encode(data, da.Compression.Default, wrapper=wrapper)
            assert zlib.decompressobj(WBITS[wrapper]).decompress(stream) == data
            info, blocks = ctx.info(), ctx.blocks()
            assert ctx.adler32_device(t.data_ptr() + big.at, big.n) == want["adler"][0]
            assert ctx.crc32_device(t.data_ptr() + big.at, big.n) == want["crc"][0]
            assert ctx.adler32_device(t.data_ptr() + ff.at, ff.n) == want["adler"][1]
            assert ctx.crc32_device(t.data_ptr() + ff.at, ff.n) == want["crc"][1]
            assert ctx.info() == info and ctx.blocks() == blocks
            assert ctx.encode(data, da.Compression.Default, wrapper=wrapper) == stream
    finally:
        ctx.close()


# ---- the batched kernels with chosen bytes ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_material():
    """the arena of cc.batch_specs(), its cases and their bytes, and per wrapper a stream of every case from Python's zlib (level 0
    for random bytes: the decode of one wave stays short)"""
    buf, cases = cc.build_arena(cc.batch_specs())
    datas = [cc.case_bytes(buf, c) for c in cases]
    streams = {w: [cc.frame(d, w, 0 if c.family == "random" else 6) for c, d in zip(cases, datas)] for w in (1, 2)}
    return buf, cases, datas, streams


def flipped(k):
    """every fourth item has one bit of its trailer flipped; which part of it alternates"""
    return (k // 4) % 2 if k % 4 == 1 else None


def with_flips(streams, wrapper):
    return [s if flipped(k) is None else cc.flip_trailer(s, wrapper, flipped(k)) for k, s in enumerate(streams)]


def stream_blob(streams):
    at, pos = [], 0
    for s in streams:
        at.append(pos)
        pos += len(s)
    return dev(b"".join(streams)), at


@pytest.mark.parametrize("wrapper", [1, 2])
def test_batched_kernels_through_verify(da, ctx, wrapper):
    buf, cases, datas, streams = batch_material()
    t = upload(buf)
    blob, at = stream_blob(streams[wrapper])
    items = [(blob.data_ptr() + a, len(s), t.data_ptr() + c.at, c.n) for a, s, c in zip(at, streams[wrapper], cases)]
    assert [k for k, c in enumerate(cases) if c.n == 0 and 0 < k < len(cases) - 1 and cases[k - 1].n and cases[k + 1].n]
    for order in (items, items[::-1]):
        rc, statuses, reps = ctx.verify_batch_device(order, wrapper)
        bad = [(k, r) for k, (s, r) in enumerate(zip(statuses, reps)) if s != da.OK or r["status"] != "OK"]
        assert rc == da.OK and not bad, (order is items, [(cc.case_id(cases[k if order is items else len(cases) - 1 - k]), r) for k, r in bad[:4]])
    # the check cannot pass vacuously: a flipped trailer is seen, and only there
    fl = with_flips(streams[wrapper], wrapper)
    blob2, at2 = stream_blob(fl)
    items2 = [(blob2.data_ptr() + a, len(s), t.data_ptr() + c.at, c.n) for a, s, c in zip(at2, fl, cases)]
    rc, statuses, reps = ctx.verify_batch_device(items2, wrapper)
    want = ["OK" if flipped(k) is None else "CHECKSUM" for k in range(len(cases))]
    assert [r["status"] for r in reps] == want, [(cc.case_id(c), r["status"], w) for c, r, w in zip(cases, reps, want) if r["status"] != w][:6]
    assert statuses == [da.OK if w == "OK" else da.E_VERIFY for w in want] and rc == da.E_VERIFY
    assert {flipped(k) for k in range(len(cases))} == {None, 0, 1}


# ---- the output side ----------------------------------------------------------------------------------------------------------------------
class OutArena:
    """output buffers of given sizes in one device tensor, filled with FILL, buffer k at OUT_OFFSETS[k % 6] behind a multiple of 16,
    CANARY everywhere else: at least 64 bytes of it in front of and behind every buffer"""

    def __init__(self, caps, offsets=OUT_OFFSETS):
        self.caps, self.at, cur = list(caps), [], 0
        for k, cap in enumerate(self.caps):
            at = cur + 64
            at += -at % 16 + offsets[k % len(offsets)]
            self.at.append(at)
            cur = at + cap
        self.host = np.full(cur + 64, CANARY, np.uint8)
        for a, cap in zip(self.at, self.caps):
            self.host[a:a + cap] = FILL
        self.t = upload(self.host)
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k] if self.caps[k] else 0

    def fetch(self):
        self.raw = self.t.cpu().numpy()

    def buf(self, k):
        return self.raw[self.at[k]:self.at[k] + self.caps[k]].tobytes()

    def guards_intact(self):
        mask = np.ones(len(self.host), bool)
        for a, cap in zip(self.at, self.caps):
            mask[a:a + cap] = False
        return bool((self.raw[mask] == CANARY).all())


@pytest.mark.parametrize("wrapper", [1, 2])
def test_batched_kernels_over_unaligned_outputs_through_inflate(da, ctx, wrapper):
    buf, cases, datas, streams = batch_material()
    for ss in (streams[wrapper], with_flips(streams[wrapper], wrapper)):
        blob, at = stream_blob(ss)
        arena = OutArena([c.n for c in cases])
        assert {a % 16 for a in arena.at} == set(OUT_OFFSETS)
        items = [(blob.data_ptr() + a, len(s), arena.ptr(k), c.n) for k, (a, s, c) in enumerate(zip(at, ss, cases))]
        rc, reps = ctx.inflate_batch_device(items, wrapper)
        arena.fetch()
        assert arena.guards_intact()
        flips = ss is not streams[wrapper]
        for k, c in enumerate(cases):
            it = reps.items[k]
            if flips and flipped(k) is not None:
                assert (it.status, reps[k]["status"]) == (da.E_DATA, "CHECKSUM"), (cc.case_id(c), reps[k])
            else:
                assert (it.status, it.out_len, reps[k]["status"]) == (da.OK, c.n, "OK"), (cc.case_id(c), reps[k])
                assert arena.buf(k) == datas[k], cc.case_id(c)
        assert rc == (da.E_DATA if flips else da.OK)


def test_single_kernels_over_an_unaligned_output_through_inflate(da, ctx):
    buf, cases, datas, streams = batch_material()
    picks = [next(k for k, c in enumerate(cases) if c.n == n) for n in (16385, 131073, 147427)]
    for wrapper in (1, 2):
        arena = OutArena([cases[k].n for k in picks], offsets=(1, 15, 3))
        for j, k in enumerate(picks):
            s = dev(streams[wrapper][k])
            rc, n, rep = ctx.inflate_device(s.data_ptr(), len(streams[wrapper][k]), arena.ptr(j), cases[k].n, wrapper)
            assert (rc, n, rep["status"]) == (da.OK, cases[k].n, "OK"), (cc.case_id(cases[k]), rep)
            bad = dev(cc.flip_trailer(streams[wrapper][k], wrapper, j % 2))
            rc, n, rep = ctx.inflate_device(bad.data_ptr(), len(streams[wrapper][k]), arena.ptr(j), cases[k].n, wrapper)
            assert (rc, rep["status"]) == (da.E_DATA, "CHECKSUM"), (cc.case_id(cases[k]), rep)
        arena.fetch()
        assert arena.guards_intact() and [arena.buf(j) for j in range(3)] == [datas[k] for k in picks]


# ---- the encode's own trailers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [1, 2])
def test_trailers_of_the_batched_encodes(da, ctx, wrapper):
    buf, cases = cc.build_arena(cc.encode_specs())
    t = upload(buf)
    ins = [(t.data_ptr() + c.at, c.n) for c in cases]
    if wrapper == 1:
        outs, lens, statuses = ctx.encode_batch_device(ins, options=da.Compression.Default, wrapper=1)
    else:
        outs, lens, statuses = ctx.encode_batch_device_gzip(ins, options=da.Compression.Default)
    assert all(s == da.OK for s in statuses)
    assert {c.at % 16 for c in cases} == {0, 1}
    for c, o, n in zip(cases, outs, lens):
        data, stream = cc.case_bytes(buf, c), o[:n].cpu().numpy().tobytes()
        if wrapper == 1:
            assert stream[-4:] == struct.pack(">I", zlib.adler32(data)), cc.case_id(c)
        else:
            assert stream[-8:] == struct.pack("<II", zlib.crc32(data), c.n), cc.case_id(c)
        d = zlib.decompressobj(WBITS[wrapper])
        assert d.decompress(stream) + d.flush() == data and d.eof and d.unused_data == b"", cc.case_id(c)


# ---- one large case -----------------------------------------------------------------------------------------------------------------------
def test_past_two_to_the_31(da, ctx):
    """The one case of the suite that is sized by a limit of the arithmetic and not by the kernels' partition: an index, a chunk
    start or an `after` that is computed in 32 bits, or in a signed type, is right for every n below 2^31 and can only go wrong
    above it -- no smaller buffer shows it.  n = 2^31 + 16384 + 5 puts a whole Adler chunk and a tail behind 2^31; n = 0xFFFEFFFF
    is the largest the entries accept, and 0xFFFF0000 must be refused.  The data is constant (0xFF, the worst case of every bound
    the Adler kernel states, then zeros), so the references are the closed forms of checksum_cases.py in Python integers and no
    host buffer of that size is made."""
    n_max = 0xFFFEFFFF
    t0 = time.time()
    t = torch.full((n_max + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    sizes = ((1 << 31) + 16384 + 5, n_max)
    for v in (0xFF, 0):
        if v == 0:
            t.zero_()
        torch.cuda.synchronize()
        for n in sizes:
            for off in ((0, 1) if n < n_max else (0,)):
                a, c = ctx.adler32_device(t.data_ptr() + off, n), ctx.crc32_device(t.data_ptr() + off, n)
                assert a == cc.adler_const(n, v), "adler, n %d, byte %02x, offset %d: %08x, want %08x" % (n, v, off, a, cc.adler_const(n, v))
                assert c == cc.crc_const(n, v), "crc, n %d, byte %02x, offset %d: %08x, want %08x" % (n, v, off, c, cc.crc_const(n, v))
    for fn in (ctx.adler32_device, ctx.crc32_device):
        with pytest.raises(da.DeflateError) as e:
            fn(t.data_ptr(), n_max + 1)
        assert e.value.code == da.E_ARG
    print("large case: %.2f s" % (time.time() - t0))
