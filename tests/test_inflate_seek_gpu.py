"""The seek points on the device (include/mi355_deflate.h mi355_inflate_seek_*): every case of inflate_seek_cases.py builds at every
spacing to the point list the rule gives, and every range read from it gets from the kernels the return value, the count, the report,
the bytes, the untouched fill behind them and the canary that the host build of the same text gives -- which are zlib's --, alone and
in batches, in one piece and in pieces; last_read() is the plan's; damage after the build and streams that give no index report what
the host build reports; the encoder's own streams read back at every level with their block tables and without; a live shard is
MI355_E_STATE; and build and reads leave the context's next encode byte-identical.
Needs a real MI355X: pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflate_seek_cases as sc
import inflseek_binding as sb

pytestmark = pytest.mark.gpu

LV = {"fast": (1, 0, 0), "default": (128, 32, 1), "best": (1768, 128, 1), "rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
KEY = ("status", "bit", "out_pos", "out_len", "n_blocks", "n_stored", "n_fixed", "n_dynamic")
FILL, CANARY = sb.FILL, 0xC3


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
    """a buffer per range in one device tensor: buffer k begins at an 8-byte boundary + its class (k % 8 unless given), is filled with
    FILL and has 64 bytes of CANARY behind it"""

    def __init__(self, lens, aligns=None):
        self.lens, self.at, host = list(lens), [], bytearray()
        for k, n in enumerate(self.lens):
            host += bytes(-len(host) % 8 + (k % 8 if aligns is None else aligns[k]))
            self.at.append(len(host))
            host += bytes([FILL]) * n + bytes([CANARY]) * sb.CANARY
        self.t = dev(host + bytes(8))
        assert self.t.data_ptr() % 8 == 0
        self.raw = None

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k]

    def fetch(self):
        self.raw = self.t.cpu().numpy().tobytes()

    def buf(self, k):
        return self.raw[self.at[k]: self.at[k] + self.lens[k]]

    def canary_ok(self, k):
        e = self.at[k] + self.lens[k]
        return self.raw[e: e + sb.CANARY] == bytes([CANARY]) * sb.CANARY


class Groups:
    """MI355_CFG_INFLATE_GROUP_BYTES for the calls inside, the default again behind them"""

    def __init__(self, da, ctx, g):
        self.da, self.ctx, self.g = da, ctx, g

    def __enter__(self):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, self.g)
        return self

    def __exit__(self, *exc):
        self.ctx.config(self.da.Context.CFG_INFLATE_GROUP_BYTES, sb.GROUP_DEFAULT)


def read_batch(ix, s_ptr, ranges, aligns=None):
    """the ranges as one batch on the device: (rc, [(status, got, report key, buffer, canary intact?)])"""
    arena = Arena([ln for _off, ln in ranges], aligns)
    rc, res = ix.read_batch_device([(off, ln, arena.ptr(k) if ln else 0) for k, (off, ln) in enumerate(ranges)], s_ptr)
    arena.fetch()
    return rc, [(st, got, key(rep), arena.buf(k), arena.canary_ok(k)) for k, (st, got, rep) in enumerate(res)]


def read_one(ix, s_ptr, off, ln, ptr_class=3):
    arena = Arena([ln], [ptr_class])
    rc, got, rep = ix.read_device(off, ln, arena.ptr(0) if ln else 0, s_ptr)
    arena.fetch()
    return rc, got, key(rep), arena.buf(0), arena.canary_ok(0)


def model(res):
    return [(rc, got, key(rep), buf, canary) for rc, got, rep, buf, canary in res]


@pytest.mark.parametrize("name", [c.name for c in sc.corpus()])
def test_every_case_matches_the_host_build(da, ctx, name):
    c = sc.by_name(name)
    s = dev(c.stream)
    found = name.startswith("text:")  # the table the device finds is the one the host's index finds
    for spacing in sc.SPACINGS:
        ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, spacing, None if found else c.table)
        host = sb.Index(c.stream, c.wrapper, c.table, spacing)
        assert ix.points() == sc.points(c.table, spacing) == host.points(), (name, spacing)
        hi = host.info()
        assert ix.info() == hi and hi["device_bytes"] == 32768 * (hi["n_points"] - 1) and key(ix.report) == key(host.report)
        ranges = sc.ranges(c, spacing)
        rc, res = read_batch(ix, s.data_ptr(), ranges)
        hrc, hres, hcounts, _stray = host.read_batch(ranges)
        assert rc == hrc == da.OK and res == model(hres), (name, spacing)
        assert ix.last_read() == hcounts and hcounts["sets"] == 1
        for (off, ln), (_st, got, _k, buf, canary) in zip(ranges, res):  # ... which are zlib's
            assert buf[:got] == c.want[off:off + ln] and got == len(c.want[off:off + ln]) and buf[got:] == bytes([FILL]) * (ln - got) and canary
        for k, (off, ln) in enumerate(ranges):  # one by one: the same, and the plan's counts
            if k % (3 if c.full else 5) == 0:
                assert read_one(ix, s.data_ptr(), off, ln) == res[k], (name, spacing, off, ln)
                assert ix.last_read() == host.read(off, ln)[5], (name, spacing, off, ln)
        ix.close()


def test_a_byte_near_the_end_costs_the_entries_behind_its_point(da, ctx):
    """a full decode and a slice would not pass: the entries decoded are those between two points, not the stream's"""
    c = sc.by_name("cut:lengths/w0")
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, sc.WIN, c.table)
    last = sc.points(c.table, sc.WIN)[-1][1]
    assert len(c.want) > 300000 and len(c.table) == 24
    for off, entries in ((len(c.want) - 70, 1), (len(c.want) - 1, 3)):
        rc, got, _k, buf, canary = read_one(ix, s.data_ptr(), off, 1)
        assert (rc, got, buf, canary) == (da.OK, 1, c.want[off:off + 1], True)
        assert ix.last_read() == dict(entries=entries, symbols=off + 1 - last, steps=entries, sets=1)
    ix.close()


@pytest.mark.parametrize("name", ["cut:lengths/w0", "cut:first_token_32768_and_1/w0", "text:l6/w0"])
def test_every_offset_class_meets_every_pointer_class(da, ctx, name):
    c = sc.by_name(name)
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, sc.WIN, c.table)
    al = sc.alignments(c, sc.WIN)
    ranges = [(off, ln) for off, ln, _a in al]
    aligns = [a for _o, _l, a in al]
    rc, res = read_batch(ix, s.data_ptr(), ranges, aligns)
    hrc, hres, _c, _s = sb.Index(c.stream, c.wrapper, c.table, sc.WIN).read_batch(ranges, aligns=aligns)
    assert rc == hrc == da.OK and res == model(hres)
    for (off, ln), (_st, got, _k, buf, canary) in zip(ranges, res):
        assert got == ln and buf == c.want[off:off + ln] and canary
    for k in range(0, len(al), 11):  # single reads at the same pointer classes
        assert read_one(ix, s.data_ptr(), ranges[k][0], ranges[k][1], aligns[k]) == res[k]
    ix.close()


@pytest.mark.parametrize("name", ["cut:lengths/w0", "text:l6/w2", "seek:oracle:pg11x3/default/w0"])
def test_a_range_longer_than_the_budget_goes_in_pieces(da, ctx, name):
    c = sc.by_name(name)
    s = dev(c.stream)
    with Groups(da, ctx, sb.GROUP_MIN):
        ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, sc.WIN, c.table)  # (built in groups of 64 KiB too)
        host = sb.Index(c.stream, c.wrapper, c.table, sc.WIN, sb.GROUP_MIN)
        assert ix.points() == host.points() == sc.points(c.table, sc.WIN) and key(ix.report) == key(host.report)
        ranges = [sc.LONG, (0, len(c.want)), (len(c.want) // 2, 70000)]
        rc, res = read_batch(ix, s.data_ptr(), ranges)
        hrc, hres, hcounts, _s = host.read_batch(ranges, group=sb.GROUP_MIN)
        assert rc == hrc == da.OK and res == model(hres) and ix.last_read() == hcounts and hcounts["sets"] >= 4
        for (off, ln), (_st, got, _k, buf, canary) in zip(ranges, res):
            assert buf[:got] == c.want[off:off + ln] and canary
        ix.close()


@pytest.mark.parametrize("name", ["cut:lengths/w1", "cut:copies_of_copies/w0", "text:l9/w0"])
def test_batches_equal_single_reads(da, ctx, name):
    c = sc.by_name(name)
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), c.wrapper, sc.WIN, c.table)
    host = sb.Index(c.stream, c.wrapper, c.table, sc.WIN)
    for ranges in sc.batches(c, sc.WIN):
        aligns = [k % 8 for k in range(len(ranges))]
        rc, res = read_batch(ix, s.data_ptr(), ranges)
        hrc, hres, hcounts, _s = host.read_batch(ranges, aligns=aligns)
        assert rc == hrc == da.OK and res == model(hres) and ix.last_read() == hcounts and hcounts["sets"] == 1
        assert [read_one(ix, s.data_ptr(), off, ln, k % 8) for k, (off, ln) in enumerate(ranges)] == res
    ix.close()


def test_damage_after_the_build_is_reported_as_the_host_build_reports_it(da, ctx):
    c = sc.by_name("cut:lengths/w0")
    s = dev(c.stream)
    ix = ctx.inflate_seek_device(s.data_ptr(), len(c.stream), 0, sc.WIN, c.table)
    host = sb.Index(c.stream, 0, c.table, sc.WIN)
    (off, ln), flips = sc.damage(c, sc.WIN)
    n_bad = 0
    for kind, bit in flips:
        m = sc.flipped(c.stream, bit)
        d = dev(m)
        ranges = [(off, ln), (0, 100), (1000, 250000)]
        with Groups(da, ctx, sb.GROUP_MIN):  # (the long range goes in pieces: a failing piece stops its range)
            rc, res = read_batch(ix, d.data_ptr(), ranges)
        hrc, hres, hcounts, _s = host.read_batch(ranges, stream=m, group=sb.GROUP_MIN)
        assert rc == hrc and res == model(hres) and ix.last_read() == hcounts, (kind, bit)
        if kind == "outside":
            assert res[0][0] == da.OK and res[0][3] == c.want[off:off + ln]
        assert res[1][0] == da.OK and res[1][3] == c.want[:100]  # a failing range disturbs no neighbour
        n_bad += res[0][0] == da.E_DATA
        one = read_one(ix, d.data_ptr(), off, ln, 0)
        assert one == res[0]
    assert n_bad >= 3


def test_streams_that_give_no_index(da, ctx):
    c = sc.by_name("cut:lengths/w0")
    t = [list(x) for x in c.table]
    t[5][1] += 1
    t[6][1] -= 1
    cases = [(c.stream, 0, [tuple(x) for x in t], "TABLE"), (c.stream[:len(c.stream) // 2], 0, c.table, None)]
    for name, at in (("cut:lengths/w1", -2), ("cut:lengths/w2", -6), ("cut:lengths/w2", -1)):
        w = sc.by_name(name)
        m = bytearray(w.stream)
        m[at] ^= 0x10
        cases.append((bytes(m), w.wrapper, w.table, "CHECKSUM"))
    L = da.load()
    for group in (sb.GROUP_DEFAULT, sb.GROUP_MIN):
        with Groups(da, ctx, group):
            for stream, wrapper, table, status in cases:
                s = dev(stream)
                host = sb.Index(stream, wrapper, table, sc.WIN, group)
                arr, nb = ctx._block_table(table)
                h, r = C.c_void_p(), da.InflateReport()
                rc = L.mi355_inflate_seek_build_device(ctx._h, s.data_ptr(), len(stream), wrapper, arr, nb, sc.WIN, C.byref(h), C.byref(r), None)
                assert rc == host.rc == da.E_DATA and h.value is None and key(r.as_dict()) == key(host.report), (status, r.as_dict(), host.report)
                assert status is None or r.as_dict()["status"] == status
                with pytest.raises(da.DeflateError) as e:
                    ctx.inflate_seek(stream, wrapper, sc.WIN, table)
                assert e.value.code == da.E_DATA


@pytest.mark.parametrize("level", list(LV))
def test_the_encoders_streams_read_back(da, ctx, level):
    data = sc.text300()
    for wrapper in (0, 1, 2):
        stream = ctx.encode(data, da.CompressionOptions(*LV[level]), wrapper=wrapper)
        info, blocks = ctx.info(), ctx.blocks()
        ranges = [(0, 100), (len(data) // 2 - 7, 65536), (len(data) - 50, 100), (len(data), 10), (12345, 0)]
        for given in (blocks, None):
            with ctx.inflate_seek(stream, wrapper, sc.WIN, given) as ix:  # host bytes: the handle keeps the stream
                i = ix.info()
                assert i["total"] == len(data) and i["device_bytes"] == 32768 * (i["n_points"] - 1) + len(stream) + 64
                if given is not None:
                    assert ix.points() == sc.points([(b["bit_start"], b["in_bytes"]) for b in blocks], sc.WIN)
                assert [ix.read(off, ln) for off, ln in ranges] == [data[off:off + ln] for off, ln in ranges] == ix.read_batch(ranges)
                assert ix.last_read()["sets"] == 1
        assert ctx.info() == info and ctx.blocks() == blocks  # last_info / last_blocks are the encode's still
    assert ctx.encode(data, da.CompressionOptions(*LV[level]), wrapper=2) == stream  # ... and the next encode is byte-identical


def test_arguments_and_state(da, ctx):
    L = da.load()
    c = sc.by_name("cut:lengths/w0")
    own = da.Context(0)  # (a context of its own: the shard is its state)
    s = dev(c.stream)
    ix = own.inflate_seek_device(s.data_ptr(), len(c.stream), 0, sc.WIN, c.table)
    out = torch.empty(1000, dtype=torch.uint8, device="cuda")
    got, r = C.c_uint64(0), da.InflateReport()
    # what a read refuses: no stream for a handle that keeps none, a length without a buffer, the host form on a device handle
    assert L.mi355_inflate_seek_read_device(ix._h, None, 0, 1000, out.data_ptr(), C.byref(got), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_seek_read_device(ix._h, s.data_ptr(), 0, 1000, None, C.byref(got), C.byref(r), None) == da.E_ARG
    assert L.mi355_inflate_seek_read(ix._h, 0, 1000, C.cast(C.create_string_buffer(1000), C.c_void_p), C.byref(got), C.byref(r)) == da.E_ARG
    n = C.c_size_t(0)
    assert L.mi355_inflate_seek_points(ix._h, None, 0, C.byref(n)) == da.E_OUT_TOO_SMALL and n.value == len(sc.points(c.table, sc.WIN))
    # a context that holds a sharded encode refuses build and read, and works again afterwards
    data = c.want[:100000]
    t = dev(data + bytes(64))
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    arr, nb = own._block_table(c.table)
    h = C.c_void_p()
    assert L.mi355_shard_begin(own._h, t.data_ptr(), len(data), 0, len(data), 0, len(data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_inflate_seek_build_device(own._h, s.data_ptr(), len(c.stream), 0, arr, nb, 0, C.byref(h), C.byref(r), None) == da.E_STATE
        assert L.mi355_inflate_seek_build(own._h, c.stream, len(c.stream), 0, arr, nb, 0, C.byref(h), C.byref(r)) == da.E_STATE
        assert L.mi355_inflate_seek_read_device(ix._h, s.data_ptr(), 0, 1000, out.data_ptr(), C.byref(got), C.byref(r), None) == da.E_STATE
        assert h.value is None
    finally:
        L.mi355_shard_end(sh)
    assert L.mi355_inflate_seek_read_device(ix._h, s.data_ptr(), 500, 1000, out.data_ptr(), C.byref(got), C.byref(r), None) == da.OK
    assert got.value == 1000 and out.cpu().numpy().tobytes() == c.want[500:1500]
    # the default spacing, and the default context (ctx == NULL)
    assert L.mi355_inflate_seek_build_device(None, s.data_ptr(), len(c.stream), 0, arr, nb, 0, C.byref(h), C.byref(r), None) == da.OK
    i = da.SeekInfo()
    assert L.mi355_inflate_seek_info(h, C.byref(i)) == da.OK and (i.spacing, i.n_points, i.total) == (1 << 20, 1, len(c.want))
    assert L.mi355_inflate_seek_read_device(h, s.data_ptr(), len(c.want) - 10, 1000, out.data_ptr(), C.byref(got), C.byref(r), None) == da.OK
    assert got.value == 10 and out.cpu().numpy().tobytes()[:10] == c.want[-10:]
    L.mi355_inflate_seek_free(h)
    ix.close()
    own.close()


def test_the_command_line_tool_reads_a_range(tmp_path):
    """examples/mi355_deflate_cli.c -d --range OFF:LEN, built with gcc and run as a process: zlib's slice, pread at the end"""
    import gzip
    import subprocess
    exe = str(tmp_path / "cli")
    subprocess.run(["gcc", "-O2", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mi355_deflate_cli.c"),
                    "-L", os.path.join(ROOT, "deflate-rs_amd"), "-lmi355deflate", "-Wl,-rpath," + os.path.join(ROOT, "deflate-rs_amd"),
                    "-o", exe], check=True)
    data = sc.text300()
    src, out = str(tmp_path / "in.gz"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(gzip.compress(data, 6, mtime=0))
    for off, ln in ((123456, 70000), (len(data) - 10, 100), (0, 1)):
        r = subprocess.run([exe, "-d", "--range", "%d:%d" % (off, ln), "-gzip", src, out], capture_output=True)
        assert r.returncode == 0, (off, ln, r.returncode, r.stderr[-2000:])
        assert open(out, "rb").read() == data[off:off + ln], (off, ln)
    for bad in ("5", "5:", ":5", "5:x"):  # not OFF:LEN: the usage text
        assert subprocess.run([exe, "-d", "--range", bad, "-gzip", src, out], capture_output=True).returncode == 2
    assert subprocess.run([exe, "-d", "--range", "0:5", "--parallel", "-gzip", src, out], capture_output=True).returncode == 2
