"""The BGZF reads on the device (include/mi355_deflate.h mi355_bgzf_index_*, mi355_bgzf_read*): for every case of bgzf_read_cases.py
the index, the return value, got, the report (all but ms), the bytes, 64 guard bytes of fill in front of and behind `out` and
mi355_bgzf_last_read are those of the host build of the same text -- which test_bgzf_read_cases.py holds against zlib --, as one
batch, alone and at the 64 KiB scratch budget; the index build refuses what the host build refuses; the host form equals the device
form and copies the touched extent only; the file of mi355_bgzf_encode_device reads back through an index of its own member table
and through a built one; the whole-file read equals mi355_inflate_members; a live shard is MI355_E_STATE.  All on one context.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import bgzf_read_cases as brc
import bgzfread_binding as hb

pytestmark = pytest.mark.gpu

CASES = brc.corpus()
KEY = ("status", "bit", "out_pos", "out_len", "n_blocks", "n_stored", "n_fixed", "n_dynamic")


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
    """the buffers of a batch in one device tensor, laid out as the host build's binding lays them out: 64 guard bytes, the range's
    bytes of fill at its class mod 16, 64 guard bytes"""

    def __init__(self, lens, aligns=None):
        self.lens = [min(n, hb.ROOM_MAX) for n in lens]
        self.at, host = hb.layout(self.lens, aligns)
        self.t = dev(host + bytes(16))
        assert self.t.data_ptr() % 16 == 0
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.lens[k]]

    def guards_ok(self, k):
        return hb.guards_intact(self.raw, self.at[k], self.lens[k])


class Budget:
    """MI355_CFG_INFLATE_GROUP_BYTES for the calls inside, the default again behind them"""

    def __init__(self, da, ctx, g):
        self.da, self.ctx, self.g = da, ctx, g

    def __enter__(self):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, self.g)
        return self

    def __exit__(self, *exc):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, hb.GROUP_DEFAULT)


def host_index(c):
    if c.index == "members":
        ix = hb.Index(members=brc.table(c), file_len=len(c.file))
        ix.file = c.file
    else:
        ix = hb.Index(file=c.file)
    assert ix.rc == hb.OK
    return ix


def device_index(da, ctx, c, d_file):
    if c.index == "members":
        ix = da.bgzf_index_from_members([dict(in_off=o, in_len=n, out_off=p, out_len=z) for o, n, p, z in brc.table(c)], len(c.file))
        ix._ctx = ctx
        return ix
    return ctx.bgzf_index_device(d_file.data_ptr(), len(c.file))


def same(c, i, dres, arena, k, hres):
    """range i of the case: the device's result (status, got, report) with buffer k of the arena against the host build's"""
    st, got, rep = dres
    hst, hgot, hrep, hbuf, hguards = hres
    assert (st, got, key(rep)) == (hst, hgot, key(hrep)), (c.name, i, rep, hrep)
    assert arena.guards_ok(k) and hguards, (c.name, i)
    buf = arena.buf(k)
    assert buf[:got] == hbuf[:got], (c.name, i)
    if st == hb.OK:
        assert buf == hbuf, (c.name, i)  # the fill behind the bytes that hold data


def run_batch(da, ctx, c, ix, hix, d_read, budget):
    with Budget(da, ctx, budget):
        arena = Arena([n for _off, n in c.ranges], c.aligns)
        rc, res = ix.read_batch_device([(off, n, arena.ptr(k) if n else 0) for k, (off, n) in enumerate(c.ranges)], d_read.data_ptr(), ctx)
        arena.fetch()
        last = ix.last_read(ctx)
    hrc, hres, hcounts = hix.read_batch(c.ranges, file=c.read_file, budget=budget, aligns=c.aligns)
    assert rc == hrc, c.name
    for i in range(len(c.ranges)):
        same(c, i, res[i], arena, i, hres[i])
    assert last == dict(hcounts, copied=0), c.name


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_host_build(da, ctx, c):
    d_file = dev(c.file)
    d_read = d_file if c.read_file == c.file else dev(c.read_file)
    ix, hix = device_index(da, ctx, c, d_file), host_index(c)
    assert [(m["in_off"], m["in_len"], m["out_off"], m["out_len"]) for m in ix.members()] == brc.table(c)
    if c.index == "build":
        assert ix.members() == hix.members() and key(ix.report) == key(hix.report)
    info = ix.info()
    info.pop("host_bytes")
    assert info == hix.info()
    # as one batch, at the case's budget and at the smallest one
    run_batch(da, ctx, c, ix, hix, d_read, c.budget)
    if c.budget != hb.GROUP_MIN:
        run_batch(da, ctx, c, ix, hix, d_read, hb.GROUP_MIN)
    # alone: a dozen of its ranges, the failing ones among them
    pick = sorted(set(list(c.expect) + list(range(0, len(c.ranges), max(1, len(c.ranges) // 12)))))
    with Budget(da, ctx, c.budget):
        for i in pick:
            off, n = c.ranges[i]
            align = 0 if c.aligns is None else c.aligns[i]
            arena = Arena([n], [align])
            rc, got, rep = ix.read_device(off, n, arena.ptr(0) if n else 0, d_read.data_ptr(), ctx)
            arena.fetch()
            last = ix.last_read(ctx)
            h = hix.read(off, n, file=c.read_file, budget=c.budget, align=align)
            assert rc == h[0]
            same(c, i, (rc, got, rep), arena, 0, h[:5])
            assert last == dict(h[5], copied=0)
    ix.close()


@pytest.mark.parametrize("name,file,pos", brc.refusals(), ids=[r[0] for r in brc.refusals()])
def test_index_build_refusals(da, ctx, name, file, pos):
    d = dev(file + b"\0")  # (a pointer for the empty file too)
    with pytest.raises(da.DeflateError) as e:
        ctx.bgzf_index_device(d.data_ptr(), len(file))
    assert e.value.code == da.E_DATA and "frame" in str(e.value).lower() and "output byte %d" % pos in str(e.value)
    with pytest.raises(da.DeflateError) as e:
        ctx.bgzf_index(file)
    assert e.value.code == da.E_DATA
    h = hb.Index(file=file)
    assert h.rc == hb.E_DATA and h.report["out_pos"] == pos


def test_host_form_equals_device_form(da, ctx):
    for c in (brc.by_name("spans/small"), brc.by_name("spans/big"), brc.by_name("boundaries"), brc.by_name("damage/member2/crc"),
              brc.by_name("damage/member3/data")):
        ix, hix = ctx.bgzf_index(c.file), host_index(c)
        tab = brc.table(c)
        for i in range(0, len(c.ranges), max(1, len(c.ranges) // 10)):
            off, n = c.ranges[i]
            if n > hb.ROOM_MAX:
                continue
            rc, got, rep, data = ix.read_raw(off, n, file=c.read_file)
            h = hix.read(off, n, file=c.read_file)
            assert (rc, got, key(rep)) == (h[0], h[1], key(h[2])) and data == h[3][:got], (c.name, i)
            ks = brc.touched(tab, off, n)
            extent = tab[ks[-1]][0] + tab[ks[-1]][1] - tab[ks[0]][0] if ks else 0
            assert ix.last_read() == dict(h[5], copied=extent), (c.name, i)
            if rc == da.OK and n <= 4096:
                assert ix.read(off, n) == data
        ok = [r for i, r in enumerate(c.ranges) if i not in c.expect and r[1] <= hb.ROOM_MAX][:40]
        if c.read_file == c.file:
            img = brc.image(c)
            assert ix.read_batch(ok) == [img[off:off + n] for off, n in ok]
        ix.close()


def test_the_encoders_file_reads_back(da, ctx):
    data = brc.imc.text(0, 200000)
    for block in (0, 4096, 100):
        n_in = len(data) if block != 100 else 5000
        d_in = dev(data[:n_in])
        cap = da.bgzf_bound(n_in, block)
        d_file = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
        _rc, flen, nm, members = ctx.encode_bgzf_device(d_in.data_ptr(), n_in, d_file.data_ptr(), cap, block_size=block)
        assert len(members) == nm
        own = da.bgzf_index_from_members(members, flen)
        built = ctx.bgzf_index_device(d_file.data_ptr(), flen)
        assert built.members() == members == own.members()
        b = block or 65280
        ranges = [(0, n_in), (b - 1, 2), (b, b), (n_in - 1, 5), (3 * b + 7, 2 * b), (n_in // 2, 4096)]
        for ix in (own, built):
            arena = Arena([n for _off, n in ranges])
            rc, res = ix.read_batch_device([(off, n, arena.ptr(k)) for k, (off, n) in enumerate(ranges)], d_file.data_ptr(), ctx, check=True)
            arena.fetch()
            for k, (off, n) in enumerate(ranges):
                want = data[:n_in][off:off + n]
                assert res[k][1] == len(want) and arena.buf(k)[:len(want)] == want and arena.guards_ok(k), (block, k)
            last = ix.last_read(ctx)
            assert last["distinct"] == sum(1 for m in members if m["out_len"]) and last["sets"] == 1
        own.close(), built.close()


def test_whole_file_read_equals_inflate_members(da, ctx):
    for file in (brc.small_file(), brc.big_file(), brc.model_file()):
        data, members = ctx.inflate_members(file)
        ix = ctx.bgzf_index(file)
        assert ix.members() == members and ix.info()["total"] == len(data)
        assert ix.read(0, len(data) + 10) == data
        full = [m for m in members if m["out_len"]]
        n, extent = len(full), full[-1]["in_off"] + full[-1]["in_len"] - full[0]["in_off"]  # (empty members are never touched)
        assert ix.last_read() == dict(distinct=n, in_place=n, scratch=0, pieces=0, sets=1, copied=extent)
        # an index made from the table of the completed members call: the same reads
        own = da.bgzf_index_from_members(members, len(file))
        assert own.read(1, len(data) - 2, ctx=ctx, file=file) == data[1:-1]
        ix.close(), own.close()


def test_stage_clocks_and_the_last_calls_are_left_alone(da, ctx):
    text = brc.imc.text(0, 50000)
    z = ctx.encode(text, da.Compression.Default)
    info, blocks = ctx.info(), ctx.blocks()
    ix = ctx.bgzf_index(brc.big_file())
    ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
    try:
        ix.read(100, 70000)
        ms = ctx.bgzf_last_read_stages()
        assert all(v > 0 for v in ms.values()), ms
    finally:
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
    ix.read(100, 10)
    assert ctx.bgzf_last_read_stages() == dict(decode=0.0, checksums=0.0, trailers=0.0)
    assert ctx.info() == info and ctx.blocks() == blocks
    assert ctx.encode(text, da.Compression.Default) == z
    ix.close()


def test_a_live_shard_is_refused(da, ctx):
    L = da.load()
    file = brc.small_file()
    d_file, out = dev(file), torch.empty(256, dtype=torch.uint8, device="cuda")
    ix = ctx.bgzf_index_device(d_file.data_ptr(), len(file))
    data = brc.imc.text(0, 100000)
    t = dev(data + bytes(64))
    sh, h, got, r = C.c_void_p(), C.c_void_p(), C.c_uint64(0), da.InflateReport()
    o = da.CompressionOptions.default().to_c()
    rng = (da.SeekRange * 1)()
    rng[0].off, rng[0].len, rng[0].out = 3, 100, out.data_ptr()
    host_out = C.create_string_buffer(100)
    assert L.mi355_shard_begin(ctx._h, t.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_bgzf_index_build_device(ctx._h, d_file.data_ptr(), len(file), C.byref(h), C.byref(r), None) == da.E_STATE
        assert L.mi355_bgzf_index_build(ctx._h, file, len(file), C.byref(h), C.byref(r)) == da.E_STATE
        assert L.mi355_bgzf_read_device(ctx._h, ix._h, d_file.data_ptr(), 3, 100, out.data_ptr(), C.byref(got), C.byref(r), None) == da.E_STATE
        assert L.mi355_bgzf_read_batch_device(ctx._h, ix._h, d_file.data_ptr(), rng, 1, None, None) == da.E_STATE
        assert L.mi355_bgzf_read(ctx._h, ix._h, file, 3, 100, C.cast(host_out, C.c_void_p), C.byref(got), C.byref(r)) == da.E_STATE
        assert h.value is None
    finally:
        L.mi355_shard_end(sh)
    assert L.mi355_bgzf_read_device(ctx._h, ix._h, d_file.data_ptr(), 3, 100, out.data_ptr(), C.byref(got), C.byref(r), None) == da.OK
    assert got.value == 100 and out.cpu().numpy().tobytes()[:100] == brc.imc.text(0, 200)[3:103]
    ix.close()


def test_the_command_line_tool_reads_a_range_of_a_bgzf_file(tmp_path):
    """examples/mi355_deflate_cli.c -d --members --range OFF:LEN, built with gcc and run as a process: the slice, pread at the end, and
    exit status 3 for a file that is not BGZF or whose touched member is damaged"""
    import subprocess
    exe = str(tmp_path / "cli")
    subprocess.run(["gcc", "-O2", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mi355_deflate_cli.c"),
                    "-L", os.path.join(ROOT, "deflate-rs_amd"), "-lmi355deflate", "-Wl,-rpath," + os.path.join(ROOT, "deflate-rs_amd"),
                    "-o", exe], check=True)
    c = brc.by_name("spans/big")
    data = brc.image(c)
    src, out = str(tmp_path / "in.gz"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(c.file)
    for off, ln in ((250, 70000), (len(data) - 10, 100), (0, 1)):
        r = subprocess.run([exe, "-d", "--members", "--range", "%d:%d" % (off, ln), src, out], capture_output=True)
        assert r.returncode == 0, (off, ln, r.returncode, r.stderr[-2000:])
        assert open(out, "rb").read() == data[off:off + ln], (off, ln)
    assert subprocess.run([exe, "-d", "--members", "--range", "0:5", "--cut", "64", src, out], capture_output=True).returncode == 2
    with open(src, "wb") as f:
        f.write(brc.imc.flip(c.file, len(c.file) - 28 - 8, 0))  # the CRC of the last data member, in front of the marker
    assert subprocess.run([exe, "-d", "--members", "--range", "0:5", src, out], capture_output=True).returncode == 0
    assert subprocess.run([exe, "-d", "--members", "--range", "%d:5" % (len(data) - 5), src, out], capture_output=True).returncode == 3
    with open(src, "wb") as f:
        f.write(c.file + b"\0")
    assert subprocess.run([exe, "-d", "--members", "--range", "0:5", src, out], capture_output=True).returncode == 3
