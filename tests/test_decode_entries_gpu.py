"""The decode-side entry points side by side (include/mi355_deflate.h mi355_deflate_verify*, mi355_inflate*): what each of them
refuses and in which order -- a bad argument before the sharded context, the sharded context before any work --, what a batch entry
does with the items it skips and how it names the first failure, and what a host entry delivers into a buffer one byte short and
in front of a damaged last block.  The later families -- members, seek points, BGZF reads -- stand in the same table, as far as an
entry has the notion: they refuse a bad argument before a context exists, so the text of the refusal is looked at where the caller
gave a context; a seek read takes its context from the handle; a batch of ranges skips nothing and names the first failing range.
One table over all of them, each on a context of its own; the results themselves are the business of the families' own suites.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import struct
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
MEMBERS = ("mi355_inflate_members", "mi355_inflate_members_device")
SEEK_BUILD = ("mi355_inflate_seek_build", "mi355_inflate_seek_build_device")
SEEK_READ = ("mi355_inflate_seek_read", "mi355_inflate_seek_read_device", "mi355_inflate_seek_read_batch_device")
BGZF_INDEX = ("mi355_bgzf_index_build", "mi355_bgzf_index_build_device")
BGZF_READ = ("mi355_bgzf_read", "mi355_bgzf_read_device", "mi355_bgzf_read_batch_device")
RANGES = ("mi355_inflate_seek_read_batch_device", "mi355_bgzf_read_batch_device")
ENTRIES = VERIFY + INFLATE + INDEX + BATCH + MEMBERS + SEEK_BUILD + SEEK_READ + BGZF_INDEX + BGZF_READ
HOST = ("mi355_inflate", "mi355_inflate_tabled", "mi355_inflate_parallel")
HOST_READS = ("mi355_inflate_members", "mi355_inflate_seek_read", "mi355_bgzf_read")
SPACING, GROUP = 32768, 65536  # a seek handle's points and the bytes of a launch set: a read crosses a point
GOT, STATUS = 77, 99            # what a range's got and status hold before a call


def dev(b):
    b = bytes(b)
    if not b:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def ptr(t):
    return t.data_ptr() if t.numel() else None


class Env:
    pass


def bgzf_member(data):
    """a gzip member with the 'BC' subfield that states its size, as bgzip writes it"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(data) + z.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(raw) + 8 - 1)
    return head + raw + struct.pack("<II", zlib.crc32(data), len(data))


def gunzip_members(file):
    """the bytes of a file of gzip members by zlib, None if it is not one"""
    out = b""
    while file:
        d = zlib.decompressobj(31)
        try:
            out += d.decompress(file)
        except zlib.error:
            return None
        if not d.eof:
            return None
        file = d.unused_data
    return out


def make_env():
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
    # a BGZF file of three members of 3000 bytes and the end-of-file marker, made on the CPU; the same file with the reserved block
    # type in its last member that holds data, and with its last bytes missing; its index (host memory: any context reads with it)
    parts = [bgzf_member(text[3000 * j:3000 * (j + 1)]) for j in range(3)] + [bgzf_member(b"")]
    assert all(len(p) <= 4096 for p in parts)
    e.bz, e.bz_data, e.bz_front, e.bz_n = b"".join(parts), text[:9000], 6000, len(parts)
    bad = bytearray(e.bz)
    bad[len(parts[0]) + len(parts[1]) + 18] |= 6
    e.bz_bad, e.bz_cut = bytes(bad), e.bz[:-3]
    e.bz_idx = C.c_void_p()
    assert e.L.mi355_bgzf_index_build(c._h, e.bz, len(e.bz), C.byref(e.bz_idx), C.byref(da.InflateReport())) == da.OK
    c.close()
    for w in (0, 1, 2):
        assert vc.zlib_accepts(EMPTY[w], b"", w) and vc.zlib_accepts(e.small_s[w], e.small, w) and vc.zlib_accepts(e.big_s[w], e.big, w)
    assert 0 < e.front <= len(e.big) and not vc.zlib_accepts(e.bad_s, e.big, 0)
    assert gunzip_members(e.bz) == e.bz_data and gunzip_members(e.bz_bad) is None and gunzip_members(e.bz_cut) is None
    e.made = {}
    return e


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.L.mi355_bgzf_index_free(e.bz_idx)


class Call:
    """one call of an entry point: the arguments behind the context in the prototype's order, by name, so that a bad call is the
    good one with an argument replaced.  A seek read has its handle ("handle") where the others have the context.  text: what a
    refused argument leaves for mi355_deflate_last_error, why: the same for the bad calls that have a text of their own"""
    text, why = None, {}

    def __init__(self, name, **args):
        self.name, self.args = name, args

    def run(self, e, h, **over):
        a = dict(self.args)
        a.update(over)
        if "handle" in a:
            h = a.pop("handle")
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


def room(device, cap):
    """cap bytes with a guard byte behind them, on the device or the host: (what keeps them alive, their pointer, held())"""
    if device:
        t = dev(bytes([GUARD]) * (cap + 1))
        return t, t.data_ptr(), lambda: t.cpu().numpy().tobytes()
    b = (C.c_uint8 * (cap + 1))()
    C.memset(b, GUARD, cap + 1)
    return b, C.cast(b, C.c_void_p), lambda: bytes(b)


def source(device, b):
    """the bytes of a stream or file where the entry wants them: (what keeps them alive, the argument)"""
    t = dev(b) if device else bytes(b)
    return t, ptr(t) if device else t


def members_call(e, name, file, data, cap, n_members=None):
    device = name.endswith("_device")
    k = Call(name)
    k.n, k.nm, k.r, k.mem = C.c_size_t(0), C.c_size_t(0), e.da.InflateReport(), (e.da.MemberInfo * 8)()
    k.keep, o, k.held = room(device, cap)
    k.src, s = source(device, file)
    k.args = dict(stream=s, stream_len=len(file), out=o, out_cap=cap, out_len=C.byref(k.n), members=k.mem, members_cap=8,
                  n_members=C.byref(k.nm), report=C.byref(k.r))
    if device:
        k.args["hip_stream"] = None
    k.bad = [dict(stream=None), dict(out=None), dict(out_len=None), dict(members=None), dict(report=None)]
    k.text = b"inflate members: bad argument"
    k.check = lambda rc: ((rc, k.n.value, k.nm.value, k.r.status, k.r.out_len) == (e.da.OK, len(data), n_members, 0, len(data)) and
                          k.held() == bytes(data) + bytes([GUARD]) * (cap + 1 - len(data)))
    return k


def seek_build_call(e, name, stream, total, wrapper):
    """with the fixture's table of two, whose second entry is a point; what the tabled calls refuse is refused in their words.
    check() frees the handle it was given"""
    device = name.endswith("_device")
    k = Call(name)
    k.seek, k.r = C.c_void_p(), e.da.InflateReport()
    k.src, s = source(device, stream)
    k.args = dict(stream=s, stream_len=len(stream), wrapper=wrapper, blocks=e.big_t[wrapper], n_blocks=2, spacing=SPACING,
                  seek=C.byref(k.seek), report=C.byref(k.r))
    if device:
        k.args["hip_stream"] = None
    k.bad = [dict(wrapper=-1), dict(wrapper=3), dict(stream=None), dict(seek=None), dict(report=None), dict(spacing=1)]
    k.text, k.why = b"inflate: bad argument", {str(dict(seek=None)): b"inflate seek: bad argument",
                                               str(dict(spacing=1)): b"inflate seek: the spacing is 0 or 32 KiB to 1 GiB"}

    def check(rc):
        info = e.da.SeekInfo()
        ok = (rc == e.da.OK and k.seek.value and k.r.status == 0 and e.L.mi355_inflate_seek_info(k.seek, C.byref(info)) == e.da.OK and
              (info.total, info.stream_len, info.wrapper, info.spacing) == (total, len(stream), wrapper, SPACING))
        e.L.mi355_inflate_seek_free(k.seek)
        k.seek.value = None
        return bool(ok)
    k.check = check
    return k


def seek_handle(e, h, device):
    """the context's handle of the raw big stream, made once per context and freed with it (shut): (handle, the stream on the device
    for a handle that keeps none, the output position of its second point)"""
    key = (h.value, device)
    if key not in e.made:
        assert e.L.mi355_deflate_ctx_config(h, e.da.Context.CFG_INFLATE_GROUP_BYTES, GROUP) == e.da.OK
        k = seek_build_call(e, SEEK_BUILD[device], e.big_s[0], len(e.big), 0)
        assert k.run(e, h) == e.da.OK
        pts, n = (e.da.SeekPoint * 64)(), C.c_size_t(0)
        assert e.L.mi355_inflate_seek_points(k.seek, pts, 64, C.byref(n)) == e.da.OK and n.value >= 2, (n.value, len(e.big))
        e.made[key] = (C.c_void_p(k.seek.value), k.src if device else None, pts[1].pos)
    return e.made[key]


def shut(e, ctx):
    """the context closed, its seek handles freed in front of it"""
    for key in [key for key in e.made if key[0] == ctx._h.value]:
        e.L.mi355_inflate_seek_free(e.made.pop(key)[0])
    ctx.close()


def range_array(e, spans, hole=None):
    """the ranges (off, len) of a batch with a buffer of len bytes and a guard byte each, marks where the call leaves got and status,
    and their report slots filled with MARK.  hole: the range without a buffer"""
    arr, reps = (e.da.SeekRange * len(spans))(), (e.da.InflateReport * len(spans))()
    C.memset(reps, MARK, C.sizeof(reps))
    bufs = [dev(bytes([GUARD]) * (n + 1)) for _, n in spans]
    for j, (off, n) in enumerate(spans):
        arr[j] = e.da.SeekRange(off, n, None if j == hole else bufs[j].data_ptr(), GOT, STATUS, 0)
    return arr, reps, bufs


def read_call(e, name, h, data, spans=None, file=None, device_handle=True):
    """a read of `data` (the big text through a seek handle of the context h, else the BGZF file's bytes through its index): one
    range, or the spans of a batch.  file: what a BGZF read decodes from, if not the file itself"""
    seek, device = name in SEEK_READ, name.endswith("_device")
    k = Call(name)
    if seek:
        handle, k.src, pos = seek_handle(e, h, device and device_handle)
        s = ptr(k.src) if k.src is not None else None
        if file is not None:
            k.src, s = source(True, file)
        head = dict(handle=handle, stream=s) if device else dict(handle=handle)
        spans = spans or [(pos - 100, 300)]
        other = seek_handle(e, h, True)[0]  # (a handle that keeps no stream: no host read of it, no device read without one)
    else:
        k.src, s = source(device, e.bz if file is None else file)
        head = dict(idx=e.bz_idx, file=s)
        spans = spans or [(2900, 3200)]
    want = [bytes(data[off:off + n]) for off, n in spans]
    if name in RANGES:
        k.arr, k.reps, k.bufs = range_array(e, spans)
        k.args = dict(head, r=k.arr, n=len(spans), reports=k.reps, hip_stream=None)
        k.bad = [dict(r=None), dict(n=1 << 31), dict(r=range_array(e, spans, hole=0)[0])]
        k.untouched = lambda: ([(r.got, r.status) for r in k.arr] == [(GOT, STATUS)] * len(spans) and
                               bytes(k.reps) == bytes([MARK]) * C.sizeof(k.reps))
        k.held = lambda j: k.bufs[j].cpu().numpy().tobytes()
        k.check = lambda rc: (rc == e.da.OK and all(
            (r.got, r.status, r.reserved, p.status, k.held(j)) == (len(w), e.da.OK, 0, 0, w + bytes([GUARD]) * (spans[j][1] + 1 - len(w)))
            for j, (r, p, w) in enumerate(zip(k.arr, k.reps, want))))
    else:
        (off, n), = spans
        k.got, k.r = C.c_uint64(GOT), e.da.InflateReport()
        k.keep, o, k.held = room(device, n)
        k.args = dict(head, off=off, len=n, out=o, got=C.byref(k.got), report=C.byref(k.r))
        if device:
            k.args["hip_stream"] = None
        k.bad = [dict(out=None), dict(got=None), dict(report=None)]
        k.check = lambda rc: ((rc, k.got.value, k.r.status) == (e.da.OK, len(want[0]), 0) and
                              k.held() == want[0] + bytes([GUARD]) * (n + 1 - len(want[0])))
    if seek:
        k.bad += [dict(handle=None), dict(stream=None) if device else dict(handle=other)]
    else:
        k.bad += [dict(idx=None), dict(file=None)]
        k.text = b"bgzf read: bad argument"
    return k


def bgzf_index_call(e, name, file):
    """check() frees the index it was given"""
    device = name.endswith("_device")
    k = Call(name)
    k.idx, k.r = C.c_void_p(), e.da.InflateReport()
    k.src, s = source(device, file)
    k.args = dict(file=s, file_len=len(file), idx=C.byref(k.idx), report=C.byref(k.r))
    if device:
        k.args["hip_stream"] = None
    k.bad = [dict(file=None), dict(idx=None), dict(report=None)]
    k.text = b"bgzf index: bad argument"

    def check(rc):
        info = e.da.BgzfInfo()
        ok = (rc == e.da.OK and k.idx.value and k.r.status == 0 and e.L.mi355_bgzf_index_info(k.idx, C.byref(info)) == e.da.OK and
              (info.total, info.n_members, info.file_len) == (len(e.bz_data), e.bz_n, len(file)))
        e.L.mi355_bgzf_index_free(k.idx)
        k.idx.value = None
        return bool(ok)
    k.check = check
    return k


def later_calls(e, name, h):
    """the valid calls of an entry of the later families on the context h"""
    if name in MEMBERS:
        return [members_call(e, name, e.bz, e.bz_data, len(e.bz_data), e.bz_n)]
    if name in SEEK_BUILD:
        out = [seek_build_call(e, name, e.big_s[w], len(e.big), w) for w in (0, 1, 2, 2)]
        out[-1].args.update(blocks=None, n_blocks=0)  # (without a table: the device finds one)
        return out
    if name in BGZF_INDEX:
        return [bgzf_index_call(e, name, e.bz)]
    data, total = (e.big, len(e.big)) if name in SEEK_READ else (e.bz_data, len(e.bz_data))
    if name in RANGES:  # the ranges in no order, one of them over the end of the data and one empty
        cross = seek_handle(e, h, True)[2] - 100 if name in SEEK_READ else 2900
        return [read_call(e, name, h, data, [(total - 50, 100), (cross, 3200), (100, 200), (7, 0)])]
    out = [read_call(e, name, h, data), read_call(e, name, h, data, [(total - 50, 100)])]
    if name == "mi355_inflate_seek_read_device":  # a handle that keeps the stream reads without one
        out.append(read_call(e, name, h, data, device_handle=False))
    return out


def good_calls(e, name, h=None):
    """valid calls of the entry, the first of them with every buffer present (the one the bad calls are made from): the small stream
    and the empty block in every frame; the tabled entries also with their table of two.  h: the context, for the seek reads, whose
    handle is the context's"""
    if name not in VERIFY + INFLATE + INDEX + BATCH:
        return later_calls(e, name, h)
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
    """(what, return code) of every bad call of the entry; where the entry leaves a text for its refusal, (return code, text) if the
    text is another"""
    k = good_calls(e, name, h)[0]
    got = []
    for over in k.bad:
        rc = k.run(e, h, **over)
        text = k.why.get(str(over), k.text)
        said = e.L.mi355_deflate_last_error(h) if text else None
        got.append((str(over), rc if said == text else (rc, said)))
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
        # (a BGZF index build has three arguments to get wrong)
        assert len(got) >= (3 if name in BGZF_INDEX else 5) and [rc for _, rc in got] == [e.da.E_ARG] * len(got), got
        k = good_calls(e, name, ctx._h)[0]  # the context is none the worse for them
        assert k.check(k.run(e, ctx._h)), name
    finally:
        shut(e, ctx)


@pytest.mark.parametrize("name", ENTRIES)
def test_sharded_context(env, name):
    """a valid call is refused with MI355_E_STATE and the one text, a bad one is a bad one still; once the shard is ended every valid
    call is served"""
    e = env
    ctx = e.da.Context(0)
    try:
        calls = good_calls(e, name, ctx._h)  # (in front of the shard: a seek read needs a handle, which a sharded context builds none of)
        sh, keep = begin_shard(e, ctx._h)
        try:
            for k in calls:
                assert k.run(e, ctx._h) == e.da.E_STATE, (name, k.args.get("wrapper"))
                assert e.L.mi355_deflate_last_error(ctx._h) == SHARDED
                if name in BATCH:
                    assert k.status() == [e.da.OK, e.da.E_UNSUPPORTED, e.da.OK] and k.untouched(1)
                    assert bytes(k.reps) == bytes([MARK]) * C.sizeof(k.reps)
                if name in RANGES:
                    assert k.untouched()
                if name in SEEK_BUILD + BGZF_INDEX:
                    assert (k.seek if name in SEEK_BUILD else k.idx).value is None
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
        for k in good_calls(e, name, ctx._h):
            assert k.check(k.run(e, ctx._h)), (name, k.args.get("wrapper"), k.args.get("stream_len"))
    finally:
        shut(e, ctx)


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


@pytest.mark.parametrize("name", HOST_READS)
def test_host_reads_one_byte_short(env, name):
    """the members call knows the file's length and says that the room is too small; a read is asked for a length and serves it"""
    e = env
    ctx = e.da.Context(0)
    try:
        if name in MEMBERS:
            cap = len(e.bz_data) - 1
            k = members_call(e, name, e.bz, e.bz_data, cap)
            assert k.run(e, ctx._h) == e.da.E_OUT_TOO_SMALL
            assert (k.n.value, k.nm.value, k.r.status, k.r.out_len) == (len(e.bz_data), e.bz_n, 0, len(e.bz_data))
            assert k.held() == e.bz_data[:cap] + bytes([GUARD])
        else:
            data = e.big if name in SEEK_READ else e.bz_data
            off = seek_handle(e, ctx._h, False)[2] - 100 if name in SEEK_READ else 2900
            k = read_call(e, name, ctx._h, data, [(off, len(data) - off - 1)])
            assert k.check(k.run(e, ctx._h))
    finally:
        shut(e, ctx)


@pytest.mark.parametrize("name", ("mi355_inflate_members", "mi355_bgzf_read"))
def test_host_reads_damaged_last_member(env, name):
    """(not the seek read: it decodes the handle's own copy of the stream, which the build has decoded whole)"""
    e = env
    ctx = e.da.Context(0)
    try:
        cap = len(e.bz_data)
        if name in MEMBERS:
            k = members_call(e, name, e.bz_bad, e.bz_data, cap)
            rc = k.run(e, ctx._h)
            got = k.n.value
            print(name, rc, got, k.nm.value, k.r.status, k.r.out_pos)
            assert k.nm.value == 3 and k.mem[2].status == k.r.status and [k.mem[j].status for j in (0, 1)] == [0, 0]
        else:
            k = read_call(e, name, ctx._h, e.bz_data, [(0, cap)], file=e.bz_bad)
            rc = k.run(e, ctx._h)
            got = k.got.value
            print(name, rc, got, k.r.status, k.r.out_pos)
        assert (rc, got, k.r.out_pos) == (e.da.E_DATA, e.bz_front, e.bz_front) and k.r.status != 0
        assert k.held() == e.bz_data[:e.bz_front] + bytes([GUARD]) * (cap + 1 - e.bz_front)
        assert e.L.mi355_deflate_last_error(ctx._h).startswith(b"inflate members: " if name in MEMBERS else b"bgzf read: range 0: ")
    finally:
        shut(e, ctx)


@pytest.mark.parametrize("name", RANGES)
def test_range_batches_name_the_first_failing_range(env, name):
    """the middle range runs into the damage: the text names it by its index, every range has its got and status and every report
    the call's time"""
    e = env
    ctx = e.da.Context(0)
    try:
        if name in SEEK_READ:
            data, file, front, said = e.big, e.bad_s, e.front, b"inflate seek: range 1: "
        else:
            data, file, front, said = e.bz_data, e.bz_bad, e.bz_front, b"bgzf read: range 1: "
        spans = [(100, 200), (front - 50, 100), (300, 100)]
        k = read_call(e, name, ctx._h, data, spans, file=file)
        rc = k.run(e, ctx._h)
        text = e.L.mi355_deflate_last_error(ctx._h)
        print(name, rc, text, [(r.got, r.status) for r in k.arr], [(p.status, p.out_pos, p.ms) for p in k.reps])
        assert rc == e.da.E_DATA and text.startswith(said), text
        assert [(r.got, r.status, r.reserved) for r in k.arr] == [(200, e.da.OK, 0), (50, e.da.E_DATA, 0), (100, e.da.OK, 0)]
        assert [p.status == 0 for p in k.reps] == [True, False, True] and k.reps[1].out_pos == front
        assert k.reps[0].ms == k.reps[1].ms == k.reps[2].ms > 0
        for j, (off, n) in enumerate(spans):
            got = k.arr[j].got
            assert k.held(j)[:got] == data[off:off + got] and k.held(j)[n:] == bytes([GUARD])
        # no report array; no range at all
        k = read_call(e, name, ctx._h, data, spans)
        assert k.run(e, ctx._h, reports=None) == e.da.OK and [(r.got, r.status) for r in k.arr] == [(n, e.da.OK) for _, n in spans]
        assert bytes(k.reps) == bytes([MARK]) * C.sizeof(k.reps)
        assert k.run(e, ctx._h, r=None, n=0) == e.da.OK
    finally:
        shut(e, ctx)


@pytest.mark.parametrize("name", SEEK_BUILD + BGZF_INDEX)
def test_failed_builds_leave_no_handle(env, name):
    """... and nothing of their staging in flight: the next valid call on the context is served"""
    e = env
    ctx = e.da.Context(0)
    try:
        if name in SEEK_BUILD:
            k = seek_build_call(e, name, e.bad_s, len(e.big), 0)
            k.seek.value, said = 1, b"inflate seek: "
        else:
            k = bgzf_index_call(e, name, e.bz_cut)
            k.idx.value, said = 1, b"bgzf index: "
        assert k.run(e, ctx._h) == e.da.E_DATA and k.r.status != 0
        assert (k.seek if name in SEEK_BUILD else k.idx).value is None
        assert e.L.mi355_deflate_last_error(ctx._h).startswith(said)
        for k in good_calls(e, name, ctx._h):
            assert k.check(k.run(e, ctx._h)), (name, k.args.get("wrapper"))
    finally:
        shut(e, ctx)
