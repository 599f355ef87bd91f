"""The members inflate on the device (include/mi355_deflate.h mi355_inflate_members*): on every case of inflate_members_cases.py and
at four span sizes mi355_inflate_members_device gives the return value, the report, the member table with its HINTED flags, the
bytes that hold data and the untouched canary of the host build, and zlib's bytes, and its find and walk kernels leave the host
build's candidates and walkers' records, span by span, those of walkers that are not on the chain included; the one-member inflate still refuses a second
member where the new call returns both; the packed gzip arena of a batched encode comes back as one file with the arena's table;
host buffers; arguments and state.  Damaged files are inputs the decoder must refuse within its bounds: nothing here provokes a fault.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_members_cases as mc
import inflmembers_binding as mb

pytestmark = pytest.mark.gpu

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


def on_chain(walks):
    """the spans of the walkers that the link from span 0 visits (how 0: linked to span `link`)"""
    k, seen = 0, []
    while k < len(walks):
        seen.append(k)
        if walks[k][4] != 0 or walks[k][5] <= k:  # (a link leads forward)
            break
        k = walks[k][5]
    return seen


def own_cap(c):
    if c.want is not None:
        return len(c.want)
    rc, n, _rep, _m, _d, _ok = mb.serial(c.stream, 0)
    return n if rc == mb.E_OUT_TOO_SMALL else 1000


@pytest.mark.parametrize("S", [16, 64, 4096, None], ids=["s16", "s64", "s4096", "default"])
def test_every_case_equals_the_host_build(da, ctx, S):
    """per case, at its own size and (at S = 64) at its short buffers: the candidates and the records of the first walk (every
    span's, on the chain or not), return code, length, report, member table, the bytes that hold data, the canary"""
    S = S or mb.span_default()
    runs = [(c, cap) for c in mc.corpus() for cap in ((own_cap(c),) + (c.caps if S == 64 else ()))]
    arena = Arena([cap for _c, cap in runs])
    ctx.config(da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, S)
    try:
        streams, got, scans = {}, [], []
        for k, (c, cap) in enumerate(runs):
            if c.name not in streams:
                streams[c.name] = dev(c.stream)
            s = streams[c.name]
            got.append(ctx.inflate_members_device(s.data_ptr() if len(c.stream) else 0, len(c.stream), arena.ptr(k), cap))
            scans.append(ctx.inflate_members_walks())
    finally:
        ctx.config(da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, mb.span_default())
    arena.fetch()
    n_hinted, want_scans, n_off_chain = 0, {}, 0
    for k, (c, cap) in enumerate(runs):
        if c.name not in want_scans:  # (an empty file has no span: nothing is found or walked)
            want_scans[c.name] = mb.scan(c.stream, S, 0) if len(c.stream) else ([], [])
        cand, walks = scans[k]
        want_cand, want_walks = want_scans[c.name]
        assert cand == want_cand, (c.name, S, cap, [(j, a, b) for j, (a, b) in enumerate(zip(cand, want_cand)) if a != b][:4])
        assert walks == want_walks, (c.name, S, cap, [(j, a, b) for j, (a, b) in enumerate(zip(walks, want_walks)) if a != b][:4])
        chain = set(on_chain(want_walks))
        n_off_chain += sum(1 for j, w in enumerate(want_walks) if j not in chain and w[4] != 3)
        rc, n, rep, members = got[k]
        want_rc, want_n, want_rep, want_members, want_data, _ok = mb.run(c.stream, S, cap)
        assert (rc, n, key(rep)) == (want_rc, want_n, key(want_rep)), (c.name, S, cap, rep, want_rep)
        assert rows(members) == want_members, (c.name, S, cap)
        held = min(n, cap)
        assert arena.buf(k)[:held] == want_data and arena.canary_ok(k), (c.name, S, cap)
        if c.want is not None:
            assert rc == (da.OK if cap >= len(c.want) else da.E_OUT_TOO_SMALL) and arena.buf(k)[:held] == c.want[:cap], (c.name, S, cap)
        else:
            assert rc in (da.E_DATA, da.E_OUT_TOO_SMALL), (c.name, S, cap)
        n_hinted += sum(m["flags"] & da.MEMBER_HINTED for m in members)
    assert n_hinted > 400
    assert S >= 4096 or n_off_chain > 50  # (walkers that hopped and that the link never visits were compared too: the small spans have them)


def test_one_member_inflate_refuses_what_the_members_call_returns(da, ctx):
    c = mc.by_name("single/gzip_second_member")
    s = dev(c.stream)
    arena = Arena([len(c.want), len(c.want)])
    rc1, _n1, rep1 = ctx.inflate_device(s.data_ptr(), len(c.stream), arena.ptr(0), len(c.want), 2)
    rc, n, rep, members = ctx.inflate_members_device(s.data_ptr(), len(c.stream), arena.ptr(1), len(c.want))
    arena.fetch()
    assert (rc1, rep1["status"]) == (da.E_DATA, "TRAILER")
    assert (rc, n, rep["status"], len(members)) == (da.OK, len(c.want), "OK", 2) and arena.buf(1) == c.want and arena.canary_ok(1)
    assert members[1]["in_off"] == members[0]["in_len"] == len(c.stream) // 2 and members[1]["out_off"] == len(c.want) // 2


@pytest.mark.parametrize("level", ["default", "rle"])
def test_the_packed_gzip_arena_is_a_file_of_members(da, ctx, level):
    """The packed encode places every region at a multiple of `align`, 4 at least, so an arena is a gzip file when no region needs
    padding.  The headers are chosen for that: a file name of 0 to 2 letters brings every member to a multiple of 4 bytes (the
    deflate data does not depend on the header), and the test asserts that the arena is dense before it inflates it."""
    opts = {"default": da.CompressionOptions(128, 32, 1), "rle": da.CompressionOptions(0, 0, 1)}[level]
    datas = [mc.text(0, 5000), b"", mc.text(7000, 70000), mc.vc.noise(1000, 9), mc.text(100, 1), mc.text(9, 300000)]
    ins = [dev(d + bytes(64))[: len(d)] for d in datas]
    blank = ctx.encode_batch_packed_device(ins, options=opts, wrapper=2, headers=[da.gzip_header()] * len(datas), align=4)
    headers = [da.gzip_header(filename=None if n % 4 == 0 else b"x" * (3 - n % 4)) for _off, n in blank.entries]
    assert len({len(h) for h in headers}) >= 2  # (some member did need a longer header)
    res = ctx.encode_batch_packed_device(ins, options=opts, wrapper=2, headers=headers, align=4)
    assert res.rc == da.OK and all(st == da.OK for st in res.statuses)
    order = sorted(range(len(datas)), key=lambda i: res.entries[i][0])  # (the regions' order in the arena is the encode's choice)
    table = [tuple(res.entries[i]) for i in order]
    ends = [off + n for off, n in table]
    assert [off for off, _n in table] == [0] + ends[:-1] and ends[-1] == res.used  # dense: byte for byte a file of members
    datas = [datas[i] for i in order]
    want = b"".join(datas)
    arena = Arena([len(want)])
    rc, n, rep, members = ctx.inflate_members_device(res.arena.data_ptr(), res.used, arena.ptr(0), len(want), check=True)
    arena.fetch()
    assert (rc, n, rep["status"]) == (da.OK, len(want), "OK") and arena.buf(0) == want and arena.canary_ok(0)
    assert [(m["in_off"], m["in_len"]) for m in members] == table  # the member table is the arena's
    assert [m["out_len"] for m in members] == [len(d) for d in datas] and not any(m["flags"] for m in members)
    # the same file through the host-buffer call, the size queried first, and the one-shot function
    blob = res.arena[: res.used].cpu().numpy().tobytes()
    assert mc.zlib_members(blob) == datas
    data, m2 = ctx.inflate_members(blob)
    assert data == want and m2 == members
    assert da.inflate_bytes(blob, 2, ctx=ctx, members=True) == want
    # an arena with padding between its regions is NOT a file: the pad bytes are the next member's FRAME
    padded = ctx.encode_batch_packed_device(ins, options=opts, wrapper=2, headers=[da.gzip_header()] * len(datas), align=64)
    rc, n, rep, members = ctx.inflate_members_device(padded.arena.data_ptr(), padded.used, arena.ptr(0), len(want))
    ptab = sorted(tuple(e) for e in padded.entries)
    k = next(i for i, (off, size) in enumerate(ptab) if ptab[i + 1][0] != off + size)  # the first region with pad behind it
    assert (rc, rep["status"], len(members)) == (da.E_DATA, "FRAME", k + 2) and members[-1]["in_off"] == sum(ptab[k])


def test_host_buffers_bgzf_and_failures(da, ctx):
    c = mc.by_name("bgzf/blocks")
    data, members = ctx.inflate_members(c.stream)
    assert data == c.want and all(m["flags"] & da.MEMBER_HINTED and m["status"] == "OK" for m in members) and len(members) == 7
    rc, n, rep, members, held = ctx.inflate_members_raw(c.stream, 100)
    assert (rc, n, held) == (da.E_OUT_TOO_SMALL, len(c.want), c.want[:100])
    c = mc.by_name("damage/bgzf/middle/crc")
    want = mb.run(c.stream, mb.span_default(), own_cap(c))
    rc, n, rep, members, held = ctx.inflate_members_raw(c.stream, own_cap(c))
    assert (rc, n, key(rep), rows(members), held) == (da.E_DATA, want[1], key(want[2]), want[3], want[4]) and rep["status"] == "CHECKSUM"
    with pytest.raises(da.DeflateError) as e:
        ctx.inflate_members(c.stream)
    assert e.value.code == da.E_DATA and "checksum" in str(e.value)
    for kw in (dict(wrapper=0, members=True), dict(wrapper=2, members=True, parallel=True), dict(wrapper=2, members=True, blocks=[])):
        with pytest.raises(ValueError):
            da.inflate_bytes(c.stream, ctx=ctx, **kw)


def test_arguments_state_table_room_and_stages(da, ctx):
    L = da.load()
    c = mc.by_name("mixed/hinted_plain_hinted")
    own = da.Context(0)  # (a context of its own: the shard is its state)
    s = dev(c.stream)
    out = torch.empty(len(c.want), dtype=torch.uint8, device="cuda")
    n, nm, r = C.c_size_t(0), C.c_size_t(0), da.InflateReport()
    tab = (da.MemberInfo * 16)()
    for bad in (0, 15, (1 << 30) + 1):
        assert L.mi355_deflate_ctx_config(own._h, da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, bad) == da.E_ARG
    args = (own._h, s.data_ptr(), len(c.stream), out.data_ptr(), len(c.want))
    assert L.mi355_inflate_members_device(*args, None, tab, 16, C.byref(nm), C.byref(r), None) == da.E_ARG  # out_len
    assert b"bad argument" in L.mi355_deflate_last_error(own._h)
    assert L.mi355_inflate_members_device(*args, C.byref(n), tab, 16, C.byref(nm), None, None) == da.E_ARG  # report
    assert L.mi355_inflate_members_device(*args, C.byref(n), None, 16, C.byref(nm), C.byref(r), None) == da.E_ARG  # table room without a table
    assert L.mi355_inflate_members_device(own._h, None, 5, out.data_ptr(), 5, C.byref(n), tab, 16, C.byref(nm), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_members_device(own._h, s.data_ptr(), len(c.stream), None, 5, C.byref(n), tab, 16, C.byref(nm), C.byref(r), None) == da.E_ARG
    # the table is cut at members_cap without an error, the count is the full one; no table and no count at all is legal
    assert L.mi355_inflate_members_device(*args, C.byref(n), tab, 4, C.byref(nm), C.byref(r), None) == da.OK
    assert (n.value, nm.value) == (len(c.want), 9) and tab[3].in_len and not tab[4].in_len and out.cpu().numpy().tobytes() == c.want
    assert L.mi355_inflate_members_device(*args, C.byref(n), None, 0, None, C.byref(r), None) == da.OK and n.value == len(c.want)
    # a context that holds a sharded encode refuses, and works again afterwards
    data = mc.text(0, 100000)
    d = dev(data + bytes(64))
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    assert L.mi355_shard_begin(own._h, d.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_inflate_members_device(*args, C.byref(n), tab, 16, C.byref(nm), C.byref(r), None) == da.E_STATE
        assert L.mi355_inflate_members(own._h, c.stream, len(c.stream), None, 0, C.byref(n), None, 0, None, C.byref(r)) == da.E_STATE
    finally:
        L.mi355_shard_end(sh)
    # the stage clocks: no launch times without them, one per launch kind used with them, the same bytes
    assert L.mi355_inflate_members_device(*args, C.byref(n), tab, 16, C.byref(nm), C.byref(r), None) == da.OK
    assert set(own.inflate_members_stages().values()) == {0.0}
    own.config(da.Context.CFG_STAGE_CLOCKS, 1)
    out.zero_()
    rc, n2, rep, members = own.inflate_members_device(s.data_ptr(), len(c.stream), out.data_ptr(), len(c.want))
    ms = own.inflate_members_stages()
    assert rc == da.OK and out.cpu().numpy().tobytes() == c.want and min(ms.values()) > 0, ms
    own.close()
    # the default context (ctx == NULL), host buffers, the size query
    assert L.mi355_inflate_members(None, c.stream, len(c.stream), None, 0, C.byref(n), None, 0, C.byref(nm), C.byref(r)) == da.E_OUT_TOO_SMALL
    assert (n.value, nm.value) == (len(c.want), 9)
