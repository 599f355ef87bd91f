"""The decode-side entry points side by side (include/mi355_deflate.h mi355_deflate_verify*, mi355_inflate*): what each of them
refuses and in which order -- a bad argument before the sharded context, the sharded context before any work --, what a batch entry
does with the items it skips and how it names the first failure, and what a host entry delivers into a buffer one byte short and
in front of a damaged last block.  One table over all of them, each on a context of its own; the results themselves are the
business of the four families' own suites.
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

import verify_cases as vc

pytestmark = pytest.mark.gpu

SHARDED = b"the context holds a sharded encode"
GUARD, MARK = 0xC3, 0xEE
# one empty fixed block, raw and in its zlib and gzip frames
EMPTY = {0: b"\x03\x00", 1: b"\x78\x9c\x03\x00\x00\x00\x00\x01",
         2: b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff\x03\x00" + bytes(8)}

VERIFY = ("mi355_deflate_verify", "mi355_deflate_verify_device")
INFLATE = ("mi355_inflate", "mi355_inflate_device", "mi355_inflate_tabled", "mi355_inflate_tabled_device", "mi355_inflate_parallel",
           "mi355_inflate_parallel_device")
INDEX = ("mi355_inflate_index", "mi355_inflate_index_device")
BATCH = ("mi355_deflate_verify_batch_device", "mi355_inflate_batch_device")
ENTRIES = VERIFY + INFLATE + INDEX + BATCH
HOST = ("mi355_inflate", "mi355_inflate_tabled", "mi355_inflate_parallel")


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def ptr(t):
    return t.data_ptr() if t.numel() else None


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """the streams every test shares: the empty block, a few hundred bytes, and the smallest encode of the text with a table of two
    entries -- its first block, and everything behind it as one entry (a coarser table is a right one)"""
    import deflate_amd as da
    e = Env()
    e.da, e.L = da, da.load()
    text = vc.pg11()
    e.text = text
    e.small = text[1000:1600]
    c = da.Context(0)
    e.small_s = {w: c.encode(e.small, da.Compression.Default, wrapper=w) for w in (0, 1, 2)}
    assert all(100 < len(s) < 600 for s in e.small_s.values())
    for size in (1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19):
        e.big = (text * 4)[:size]
        c.encode(e.big, da.Compression.Default)
        if len(c.blocks()) >= 2:
            break
    e.big_s, e.big_t = {}, {}
    for w in (0, 1, 2):
        e.big_s[w] = c.encode(e.big, da.Compression.Default, wrapper=w)
        bl = c.blocks()
        assert len(bl) >= 2 and sum(b["in_bytes"] for b in bl) == len(e.big)
        t = (da.BlockInfo * 2)()
        t[0].bit_start, t[0].in_bytes = bl[0]["bit_start"], bl[0]["in_bytes"]
        t[1].bit_start, t[1].in_bytes = bl[1]["bit_start"], len(e.big) - bl[0]["in_bytes"]
        e.big_t[w] = t
        if w == 0:  # the raw stream with the reserved block type in the header of its last block
            e.front = len(e.big) - bl[-1]["in_bytes"]
            bad = bytearray(e.big_s[0])
            for q in (bl[-1]["bit_start"] + 1, bl[-1]["bit_start"] + 2):
                bad[q >> 3] |= 1 << (q & 7)
            e.bad_s = bytes(bad)
    c.close()
    for w in (0, 1, 2):
        assert vc.zlib_accepts(EMPTY[w], b"", w) and vc.zlib_accepts(e.small_s[w], e.small, w) and vc.zlib_accepts(e.big_s[w], e.big, w)
    assert 0 < e.front <= len(e.big) and not vc.zlib_accepts(e.bad_s, e.big, 0)
    return e


class Call:
    """one call of an entry point: the arguments behind the context in the prototype's order, by name, so that a bad call is the
    good one with an argument replaced"""

    def __init__(self, name, **args):
        self.name, self.args = name, args

    def run(self, e, h, **over):
        a = dict(self.args)
        a.update(over)
        return getattr(e.L, self.name)(h, *a.values())


def verify_call(e, name, stream, data, wrapper, table=None):
    k = Call(name)
    k.r = e.da.VerifyReport()
    if name.endswith("_device"):
        k.keep = (dev(stream), dev(data))
        s, d = ptr(k.keep[0]), ptr(k.keep[1])
    else:
        s, d = bytes(stream), bytes(data)
    k.args = dict(stream=s, stream_len=len(stream), inp=d, in_len=len(data), wrapper=wrapper, blocks=table, n_blocks=len(table) if table else 0,
                  report=C.byref(k.r))
    if name.endswith("_device"):
        k.args["hip_stream"] = None
    k.bad = [dict(wrapper=-1), dict(wrapper=3), dict(stream=None), dict(inp=None), dict(report=None)]
    k.check = lambda rc: (rc, k.r.status) == (e.da.OK, 0)
    return k


def inflate_call(e, name, stream, data, wrapper, cap, table=None):
    """cap bytes of buffer with a guard byte behind them; held(): what the call left in the buffer, the guard included"""
    k = Call(name)
    k.n, k.r = C.c_size_t(0), e.da.InflateReport()
    if name.endswith("_device"):
        k.keep = (dev(stream), dev(bytes([GUARD]) * (cap + 1)))
        s, o = ptr(k.keep[0]), k.keep[1].data_ptr() if cap else None
        k.held = lambda: k.keep[1].cpu().numpy().tobytes()
    else:
        k.keep = (C.c_uint8 * (cap + 1))()
        C.memset(k.keep, GUARD, cap + 1)
        s, o = bytes(stream), C.cast(k.keep, C.c_void_p) if cap else None
        k.held = lambda: bytes(k.keep)
    k.args = dict(stream=s, stream_len=len(stream), wrapper=wrapper)
    if "_tabled" in name:
        k.args.update(blocks=table, n_blocks=len(table) if table else 0)
    k.args.update(out=o, out_cap=cap, out_len=C.byref(k.n), report=C.byref(k.r))
    if name.endswith("_device"):
        k.args["hip_stream"] = None
    k.bad = [dict(wrapper=-1), dict(wrapper=3), dict(stream=None), dict(out=None), dict(out_len=None), dict(report=None)]
    k.check = lambda rc: ((rc, k.n.value, k.r.status, k.r.out_len) == (e.da.OK, len(data), 0, len(data)) and
                          k.held() == bytes(data) + bytes([GUARD]) * (cap + 1 - len(data)))
    return k


def index_call(e, name, stream, data, wrapper, cap=64):
    k = Call(name)
    k.n, k.r, k.blocks = C.c_size_t(0), e.da.InflateReport(), (e.da.BlockInfo * cap)()
    if name.endswith("_device"):
        k.keep = dev(stream)
        s = ptr(k.keep)
    else:
        s = bytes(stream)
    k.args = dict(stream=s, stream_len=len(stream), wrapper=wrapper, blocks=k.blocks, cap=cap, n_blocks=C.byref(k.n), report=C.byref(k.r))
    if name.endswith("_device"):
        k.args["hip_stream"] = None
    k.bad = [dict(wrapper=-1), dict(wrapper=3), dict(stream=None), dict(blocks=None), dict(n_blocks=None), dict(report=None)]
    k.check = lambda rc: ((rc, k.r.status) == (e.da.OK, 0) and 1 <= k.n.value <= cap and
                          sum(k.blocks[j].in_bytes for j in range(k.n.value)) == len(data))
    return k


def batch_call(e, name, streams, datas, wrapper, skipped=(1,), hole=None):
    """three items; the skipped ones carry a status, a length without a pointer (nobody looks) and 77 where inflate would write the
    length; the report slots are filled with MARK.  hole: the pointer of item 0 that is missing"""
    verify = "verify" in name
    k = Call(name)
    n = len(streams)
    k.items = (e.da.BatchItem * n)()
    k.reps = ((e.da.VerifyReport if verify else e.da.InflateReport) * n)()
    C.memset(k.reps, MARK, C.sizeof(k.reps))
    k.keep = [(dev(s), dev(d) if verify else dev(bytes([GUARD]) * (len(d) + 1))) for s, d in zip(streams, datas)]
    for j, (s, d) in enumerate(k.keep):
        it = k.items[j]
        if verify:
            it.out, it.out_len, it.out_cap, it.in_, it.in_len = ptr(s), s.numel(), s.numel(), ptr(d), d.numel()
        else:
            it.in_, it.in_len, it.out, it.out_cap, it.out_len = ptr(s), s.numel(), ptr(d) if len(datas[j]) else None, len(datas[j]), 77
        if j in skipped:
            it.status, it.in_, it.in_len = e.da.E_UNSUPPORTED, None, 5
    if hole:
        setattr(k.items[0], hole, None)
    k.args = dict(items=k.items, n_items=n, wrapper=wrapper, reports=k.reps, hip_stream=None)
    k.bad = [dict(wrapper=-1), dict(wrapper=3), dict(items=None)]
    k.status = lambda: [k.items[j].status for j in range(n)]
    k.untouched = lambda j: ((k.items[j].status, k.items[j].in_len) == (e.da.E_UNSUPPORTED, 5) and
                             bytes(k.reps[j]) == bytes([MARK]) * C.sizeof(k.reps[j]) and
                             (verify or (k.items[j].out_len == 77 and
                                         k.keep[j][1].cpu().numpy().tobytes() == bytes([GUARD]) * (len(datas[j]) + 1))))
    k.answered = lambda j: (k.items[j].status == e.da.OK and k.reps[j].status == 0 and
                            (verify or (k.items[j].out_len == len(datas[j]) and
                                        k.keep[j][1].cpu().numpy().tobytes() == bytes(datas[j]) + bytes([GUARD]))))
    k.check = lambda rc: rc == e.da.OK and k.answered(0) and k.untouched(1) and k.answered(2)
    return k


def good_calls(e, name):
    """valid calls of the entry, the first of them with every buffer present (the one the bad calls are made from): the small stream
    and the empty block in every frame; the tabled entries also with their table of two"""
    out = []
    for w in (0, 1, 2):
        if name in BATCH:
            out.append(batch_call(e, name, [e.small_s[w], EMPTY[w], EMPTY[w]], [e.small, b"", b""], w))
            continue
        for stream, data in ((e.small_s[w], e.small), (EMPTY[w], b"")):
            if name in VERIFY:
                out.append(verify_call(e, name, stream, data, w))
            elif name in INDEX:
                out.append(index_call(e, name, stream, data, w))
            else:
                out.append(inflate_call(e, name, stream, data, w, len(data)))  # (a tabled entry without a table: the one-wave call)
        if name in VERIFY:
            out.append(verify_call(e, name, e.big_s[w], e.big, w, e.big_t[w]))
        if "_tabled" in name:
            out.append(inflate_call(e, name, e.big_s[w], e.big, w, len(e.big), e.big_t[w]))
    if "_tabled" in name:  # the bad calls of a tabled entry are calls with a table
        out.insert(0, out.pop(2))
    return out


def bad_calls(e, name, h, sharded):
    """(what, return code) of every bad call of the entry"""
    k = good_calls(e, name)[0]
    got = [(str(over), k.run(e, h, **over)) for over in k.bad]
    if name in BATCH:
        w = k.args["wrapper"]
        for hole in ("in_", "out"):
            b = batch_call(e, name, [e.small_s[w]] * 3, [e.small] * 3, w, hole=hole)
            got.append((hole, b.run(e, h)))
    if name == "mi355_deflate_verify_device" or (name == "mi355_deflate_verify" and not sharded):
        got.append(("n_blocks without blocks", k.run(e, h, blocks=None, n_blocks=1)))
    return got


def begin_shard(e, h):
    """a sharded encode held by the context, the way tests/test_inflate_gpu.py makes one"""
    t = dev(e.text + bytes(64))
    sh = C.c_void_p()
    o = e.da.CompressionOptions.default().to_c()
    assert e.L.mi355_shard_begin(h, t.data_ptr(), len(e.text), 0, len(e.text), 0, len(e.text), C.byref(o), None, C.byref(sh)) == e.da.OK
    return sh, t


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_arguments(env, name):
    e = env
    ctx = e.da.Context(0)
    try:
        got = bad_calls(e, name, ctx._h, False)
        assert len(got) >= 5 and [rc for _, rc in got] == [e.da.E_ARG] * len(got), got
        k = good_calls(e, name)[0]  # the context is none the worse for them
        assert k.check(k.run(e, ctx._h)), name
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ENTRIES)
def test_sharded_context(env, name):
    """a valid call is refused with MI355_E_STATE and the one text, a bad one is a bad one still; once the shard is ended every valid
    call is served"""
    e = env
    ctx = e.da.Context(0)
    try:
        sh, keep = begin_shard(e, ctx._h)
        try:
            for k in good_calls(e, name):
                assert k.run(e, ctx._h) == e.da.E_STATE, (name, k.args["wrapper"])
                assert e.L.mi355_deflate_last_error(ctx._h) == SHARDED
                if name in BATCH:
                    assert k.status() == [e.da.OK, e.da.E_UNSUPPORTED, e.da.OK] and k.untouched(1)
                    assert bytes(k.reps) == bytes([MARK]) * C.sizeof(k.reps)
            got = bad_calls(e, name, ctx._h, True)
            assert [rc for _, rc in got] == [e.da.E_ARG] * len(got), got
            if name == "mi355_deflate_verify":
                # (this entry leaves the table's pair of arguments to its worker, behind its copies: the context is looked at first)
                k = good_calls(e, name)[0]
                assert k.run(e, ctx._h, blocks=None, n_blocks=1) == e.da.E_STATE
            if name in BATCH:
                # a batch without an active item is refused too: the context is looked at before the list of active items
                k = batch_call(e, name, [EMPTY[0]] * 3, [b""] * 3, 0, skipped=(0, 1, 2))
                assert k.run(e, ctx._h) == e.da.E_STATE and e.L.mi355_deflate_last_error(ctx._h) == SHARDED
                assert k.run(e, ctx._h, items=None, n_items=0) == e.da.E_STATE
        finally:
            e.L.mi355_shard_end(sh)
        for k in good_calls(e, name):
            assert k.check(k.run(e, ctx._h)), (name, k.args["wrapper"], k.args["stream_len"] if name not in BATCH else None)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", BATCH)
def test_batch_entries_skip_and_name_by_the_callers_index(env, name):
    e = env
    verify = "verify" in name
    ctx = e.da.Context(0)
    try:
        # the last item fails: the text names it by its place in the caller's array, 2, not in the list of active items, 1
        wrong = e.small[:-1] + b"#"
        k = batch_call(e, name, [e.small_s[0], e.small_s[0], e.small_s[0][:-8] if not verify else e.small_s[0]],
                       [e.small, e.small, wrong if verify else e.small], 0)
        want = e.da.E_VERIFY if verify else e.da.E_DATA
        assert k.run(e, ctx._h) == want
        text = e.L.mi355_deflate_last_error(ctx._h)
        assert text.startswith(b"verify: item 2: " if verify else b"inflate: item 2: "), text
        assert k.answered(0) and k.untouched(1) and k.items[2].status == want and k.reps[2].status != 0
        assert k.reps[0].ms == k.reps[2].ms > 0
        # no report array; every item skipped; no item at all
        k = batch_call(e, name, [e.small_s[1]] * 3, [e.small] * 3, 1)
        assert k.run(e, ctx._h, reports=None) == e.da.OK and k.status() == [e.da.OK, e.da.E_UNSUPPORTED, e.da.OK]
        assert bytes(k.reps) == bytes([MARK]) * C.sizeof(k.reps)
        k = batch_call(e, name, [e.small_s[2]] * 3, [e.small] * 3, 2, skipped=(0, 1, 2))
        assert k.run(e, ctx._h) == e.da.OK and all(k.untouched(j) for j in range(3))
        assert k.run(e, ctx._h, items=None, n_items=0) == e.da.OK
    finally:
        ctx.close()


def host_call(e, name, stream, cap):
    return inflate_call(e, name, stream, e.big, 0, cap, e.big_t[0] if "_tabled" in name else None)


@pytest.mark.parametrize("name", HOST)
def test_host_entries_one_byte_short(env, name):
    e = env
    ctx = e.da.Context(0)
    try:
        cap = len(e.big) - 1
        k = host_call(e, name, e.big_s[0], cap)
        assert k.run(e, ctx._h) == e.da.E_OUT_TOO_SMALL
        assert (k.n.value, k.r.status, k.r.out_len) == (len(e.big), 0, len(e.big))
        assert k.held() == e.big[:cap] + bytes([GUARD])
    finally:
        ctx.close()


@pytest.mark.parametrize("name", HOST)
def test_host_entries_damaged_last_block(env, name):
    e = env
    ref = zlib.decompressobj(-15).decompress(e.big_s[0])
    ctx = e.da.Context(0)
    try:
        cap = len(e.big)
        k = host_call(e, name, e.bad_s, cap)
        assert k.run(e, ctx._h) == e.da.E_DATA
        print(name, k.n.value, e.front, k.r.status, k.r.out_pos)
        assert (k.n.value, k.r.out_pos) == (e.front, e.front) and k.r.status != 0
        assert k.held() == ref[:e.front] + bytes([GUARD]) * (cap + 1 - e.front)
    finally:
        ctx.close()
