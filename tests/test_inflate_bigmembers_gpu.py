"""The large plain members of the members inflate on the device (include/mi355_deflate.h mi355_inflate_members*,
MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES): on every case of inflate_bigmembers_cases.py, at index spans of 256 and 4096 bytes, with
groups of 64 KiB and of the default size and the threshold at 1 KiB, mi355_inflate_members_device gives the return value, the
report, the member table with its flags, the bytes that hold data and the untouched canary of the host build of tests/inflbig, zlib's
bytes, and the host build's six counters -- on a valid file the expected number of parallel members among them; with the setting at
0 the same results and no parallel member; host buffers; the packed gzip arena of a batched encode comes back with every member
decoded in parallel.  Damaged files are inputs the decoder must refuse within its bounds: nothing here provokes a fault.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_bigmembers_cases as bc
import inflbig_binding as bb
import inflmembers_binding as mb

pytestmark = pytest.mark.gpu

KEY = ("status", "bit", "out_pos", "out_len", "n_blocks", "n_stored", "n_fixed", "n_dynamic")
FILL, CANARY = 0xA5, 0xC3
T = bc.THRESHOLD
INDEX_SPAN_DEFAULT = 16384


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


def rows(members):
    return [(m["in_off"], m["in_len"], m["out_off"], m["out_len"], m["flags"], m["status"]) for m in members]


class Arena:
    """output buffers of given sizes in one device tensor: buffer k begins at an 8-byte boundary + k % 8, is filled with FILL and
    has 64 bytes of CANARY behind it"""

    def __init__(self, caps):
        self.caps, self.at, host = list(caps), [], bytearray()
        for k, cap in enumerate(self.caps):
            host += bytes(-len(host) % 8 + k % 8)
            self.at.append(len(host))
            host += bytes([FILL]) * cap + bytes([CANARY]) * mb.CANARY
        self.t = dev(host + bytes(8))
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k] if self.caps[k] else 0

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.caps[k]]

    def canary_ok(self, k):
        e = self.at[k] + self.caps[k]
        return self.raw[e: e + mb.CANARY] == bytes([CANARY]) * mb.CANARY


def own_cap(c):
    if c.want is not None:
        return len(c.want)
    rc, n, _rep, _m, _d, _ok = mb.serial(c.stream, 0)
    return n if rc == mb.E_OUT_TOO_SMALL else 70000


class settings:
    """the three settings of a test, and the defaults back behind it"""

    def __init__(self, da, ctx, threshold, index_span, group_bytes):
        self.da, self.ctx, self.v = da, ctx, (threshold, index_span, group_bytes)

    def put(self, v):
        K = self.da.Context
        for k, x in zip((K.CFG_INFLATE_MEMBER_PARALLEL_BYTES, K.CFG_INFLATE_INDEX_SPAN_BYTES, K.CFG_INFLATE_GROUP_BYTES), v):
            self.ctx.config(k, x)

    def __enter__(self):
        self.put(self.v)

    def __exit__(self, *exc):
        self.put((65536, INDEX_SPAN_DEFAULT, bb.GROUP_DEFAULT))


def run_all(ctx, runs):
    """[(case, cap)] through mi355_inflate_members_device: the results, the counters, the arena fetched"""
    arena = Arena([cap for _c, cap in runs])
    streams, got, counters = {}, [], []
    for k, (c, cap) in enumerate(runs):
        if c.name not in streams:
            streams[c.name] = dev(c.stream)
        got.append(ctx.inflate_members_device(streams[c.name].data_ptr(), len(c.stream), arena.ptr(k), cap))
        counters.append(ctx.inflate_members_last_parallel())
    arena.fetch()
    return got, counters, arena


@pytest.mark.parametrize("S,g", [(256, bc.GROUP_SMALL), (256, bb.GROUP_DEFAULT), (4096, bc.GROUP_SMALL), (4096, bb.GROUP_DEFAULT)],
                         ids=["s256-g64k", "s256-gdefault", "s4096-g64k", "s4096-gdefault"])
def test_every_case_equals_the_host_build(da, ctx, S, g):
    """per case, at its own size and (at the first setting) at its short buffers: return code, length, report, member table with its
    flags, the bytes that hold data, the canary, and the six counters"""
    short = (S, g) == (256, bc.GROUP_SMALL)
    runs = [(c, cap) for c in bc.corpus() for cap in ((own_cap(c),) + (c.caps if short else ()))]
    with settings(da, ctx, T, S, g):
        got, counters, arena = run_all(ctx, runs)
    n_parallel = 0
    for k, (c, cap) in enumerate(runs):
        rc, n, rep, members = got[k]
        (want_rc, want_n, want_rep, want_members, want_data, _ok), want_st = bb.run(c.stream, mb.span_default(), cap, T, S, g)
        assert (rc, n, key(rep)) == (want_rc, want_n, key(want_rep)), (c.name, S, g, cap, rep, want_rep)
        assert rows(members) == want_members, (c.name, S, g, cap)
        held = min(n, cap)
        assert arena.buf(k)[:held] == want_data and arena.canary_ok(k), (c.name, S, g, cap)
        assert counters[k] == want_st, (c.name, S, g, cap)
        if c.want is not None:
            assert rc == (da.OK if cap >= len(c.want) else da.E_OUT_TOO_SMALL) and arena.buf(k)[:held] == c.want[:cap], (c.name, S, g, cap)
            assert counters[k]["parallel"] == c.expect, (c.name, S, g, cap, counters[k])
        else:
            assert rc == da.E_DATA, (c.name, S, g, cap)
        n_parallel += counters[k]["parallel"]
    assert n_parallel > 100


def test_switched_off_the_results_are_the_same_and_nothing_is_parallel(da, ctx):
    runs = [(c, len(c.want)) for c in bc.valid()]
    with settings(da, ctx, 0, 256, bc.GROUP_SMALL):
        off, counters, arena = run_all(ctx, runs)
    assert not any(v for st in counters for v in st.values())
    with settings(da, ctx, T, 256, bc.GROUP_SMALL):
        on, counters_on, arena_on = run_all(ctx, runs)
    for k, (c, cap) in enumerate(runs):
        assert (off[k][0], off[k][1], key(off[k][2]), rows(off[k][3])) == (on[k][0], on[k][1], key(on[k][2]), rows(on[k][3])), c.name
        assert arena.buf(k) == arena_on.buf(k) == c.want and arena.canary_ok(k) and arena_on.canary_ok(k), c.name
        assert counters_on[k]["parallel"] == c.expect, c.name


def test_host_buffers(da, ctx):
    with settings(da, ctx, T, 256, bc.GROUP_SMALL):
        for name in ("valid/plain3", "valid/bgzf_plain_bgzf", "damage/middle/far_distance"):
            c = bc.by_name(name)
            cap = own_cap(c)
            (want_rc, want_n, want_rep, want_members, want_data, _ok), want_st = bb.run(c.stream, mb.span_default(), cap, T, 256, bc.GROUP_SMALL)
            rc, n, rep, members, held = ctx.inflate_members_raw(c.stream, cap)
            assert (rc, n, key(rep), rows(members), held) == (want_rc, want_n, key(want_rep), want_members, want_data), name
            assert ctx.inflate_members_last_parallel() == want_st, name
        c = bc.by_name("valid/plain3")
        assert da.inflate_bytes(c.stream, 2, ctx=ctx, members=True) == c.want
        # a call refused for its arguments leaves no other call's counters behind it
        assert any(ctx.inflate_members_last_parallel().values())
        r = da.InflateReport()
        assert da.load().mi355_inflate_members(ctx._h, c.stream, len(c.stream), None, 0, None, None, 0, None, C.byref(r)) == da.E_ARG
        assert not any(ctx.inflate_members_last_parallel().values())


def test_the_packed_gzip_arena_comes_back_with_every_member_parallel(da, ctx):
    """mi355_deflate_encode_batch_packed_device, gzip members at align 4, then mi355_inflate_members_device: the inputs, and all
    eight members by the parallel path.  The headers make the arena dense, as in test_inflate_members_gpu.py."""
    datas = [bc.text(100000 * k, 128 << 10) for k in range(8)]
    ins = [dev(d + bytes(64))[: len(d)] for d in datas]
    opts = da.CompressionOptions(128, 32, 1)
    blank = ctx.encode_batch_packed_device(ins, options=opts, wrapper=2, headers=[da.gzip_header()] * len(datas), align=4)
    headers = [da.gzip_header(filename=None if n % 4 == 0 else b"x" * (3 - n % 4)) for _off, n in blank.entries]
    res = ctx.encode_batch_packed_device(ins, options=opts, wrapper=2, headers=headers, align=4)
    assert res.rc == da.OK and all(st == da.OK for st in res.statuses)
    order = sorted(range(len(datas)), key=lambda i: res.entries[i][0])
    table = [tuple(res.entries[i]) for i in order]
    ends = [off + n for off, n in table]
    assert [off for off, _n in table] == [0] + ends[:-1] and ends[-1] == res.used  # dense: byte for byte a file of members
    want = b"".join(datas[i] for i in order)
    arena = Arena([len(want)])
    with settings(da, ctx, T, INDEX_SPAN_DEFAULT, bb.GROUP_DEFAULT):
        rc, n, rep, members = ctx.inflate_members_device(res.arena.data_ptr(), res.used, arena.ptr(0), len(want), check=True)
        st = ctx.inflate_members_last_parallel()
    arena.fetch()
    assert (rc, n, rep["status"]) == (da.OK, len(want), "OK") and arena.buf(0) == want and arena.canary_ok(0)
    assert [(m["in_off"], m["in_len"]) for m in members] == table and not any(m["flags"] for m in members)
    assert (st["parallel"], st["handed"]) == (8, 0) and st["entries"] >= 8 and st["sets"] == 1, st
