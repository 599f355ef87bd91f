"""The gzip forms of the batched encode (mi355_deflate_encode_batch[_device]_gzip) on the GPU: every item byte for byte what
mi355_deflate_encode_gzip and the oracle give for it alone with its own header, whatever the batch around it and wherever the
header's length puts the start of the stream; the routing is that of the zlib batch; the device entry; the errors.  pytest -m gpu."""
import ctypes as C
import glob
import gzip
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import datagen
import oracle_binding as ob

pytestmark = pytest.mark.gpu

FIX = os.path.join(HERE, "golden", "ref_inputs")
LV = {"fast": (1, 0, 0), "default": (128, 32, 1), "best": (1768, 128, 1), "rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
E_ARG, E_OUT_TOO_SMALL, E_UNSUPPORTED = -1, -2, -4


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


def fixtures():
    out = []
    for p in sorted(glob.glob(os.path.join(FIX, "*")) + glob.glob(os.path.join(FIX, "afl", "**", "*"), recursive=True)):
        if os.path.isfile(p):
            out.append(open(p, "rb").read())
    return out


def mixed_items():
    t = datagen.text_like(3 << 20, 11)
    return ([b"", b"a", b"ab", b"abc", t[:32767], t[1:32769], t[2:32771]] + fixtures() +
            [t[:1 << 20], t[5:5 + (2 << 20)], t, bytes(1 << 20), datagen.rng_bytes(100000, 3)])


def named_headers(da, n):
    """one header per item: file names of varying length (so the streams start on every byte of a word), an mtime, a comment now and then"""
    hs = []
    for k in range(n):
        name = b"item-%d" % k + b"x" * (k % 7) + b".txt"
        hs.append(da.gzip_header(filename=name, mtime=1700000000 + k, comment=(b"c" * (k % 5)) if k % 3 == 0 else None))
    return hs


def header_of(da, headers, k):
    if headers is None:
        return da.BLANK_GZIP_HEADER
    return headers if isinstance(headers, bytes) else headers[k]


def raw_batch(da, ctx, datas, o, hdrs, n_hdrs, caps=None, hlens=None, sentinel=None):
    """the raw host entry: (rc, outputs, statuses, out_lens); hdrs: a GzipHeader array or None"""
    L = da.load()
    items = (da.BatchItem * max(len(datas), 1))()
    bufs = []
    for k, d in enumerate(datas):
        cap = L.mi355_deflate_bound_ex(len(d), 2, hlens[k] if hlens else 10, 0) if caps is None else caps[k]
        out = (C.c_uint8 * max(cap, 1))()
        bufs.append((d, out))
        items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
        items[k].in_len = len(d)
        items[k].out = C.cast(out, C.c_void_p)
        items[k].out_cap = cap
        if sentinel is not None:
            items[k].status = sentinel
    rc = L.mi355_deflate_encode_batch_gzip(ctx._h, items, len(datas), C.byref(o), hdrs, n_hdrs)
    outs = [bytes(memoryview(bufs[k][1])[: items[k].out_len]) if items[k].status == 0 else None for k in range(len(datas))]
    return rc, outs, [items[k].status for k in range(len(datas))], [items[k].out_len for k in range(len(datas))]


def header_array(da, hs):
    arr = (da.GzipHeader * max(len(hs), 1))()
    for k, h in enumerate(hs):
        arr[k].hdr = h
        arr[k].hdr_len = len(h)
    return arr


def check_parity(da, ctx, level, headers_kind):
    c, l, m = LV[level]
    opts = da.CompressionOptions(c, l, m)
    datas = mixed_items()
    headers = {"blank": None, "shared": da.gzip_header(filename=b"shared-name.bin", mtime=1234567),
               "per_item": named_headers(da, len(datas))}[headers_kind]
    outs = ctx.encode_batch_gzip(datas, opts, headers)
    assert len(outs) == len(datas)
    for k, d in enumerate(datas):
        h = header_of(da, headers, k)
        assert outs[k] == ctx.encode_gzip(d, opts, h), "item %d (%d bytes) differs from its one-input call" % (k, len(d))
        assert outs[k] == ob.encode_gzip(d, h, opts=ob.make_opts(c, l, m, 0)), "item %d differs from the oracle" % k
        assert gzip.decompress(outs[k]) == d  # (checks CRC-32 and the length itself)


@pytest.mark.parametrize("level", list(LV))
def test_blank_header_matches_single_calls_and_oracle(da, ctx, level):
    check_parity(da, ctx, level, "blank")


@pytest.mark.parametrize("headers_kind", ["shared", "per_item"])
@pytest.mark.parametrize("level", ["default", "fast"])
def test_headers_match_single_calls_and_oracle(da, ctx, level, headers_kind):
    check_parity(da, ctx, level, headers_kind)


def test_module_level_functions(da, ctx):
    t = datagen.text_like(90000, 8)
    datas = [t[:30000], t[30000:], b""]
    hs = named_headers(da, 3)
    assert da.deflate_bytes_gzip_batch(datas, ctx) == [ctx.encode_gzip(d) for d in datas]
    assert da.deflate_bytes_gzip_batch_conf(datas, da.Compression.Fast, hs, ctx) == [
        ctx.encode_gzip(d, da.Compression.Fast, h) for d, h in zip(datas, hs)]


def test_stream_starts_on_every_byte_of_a_word(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    rnd = random.Random(17)
    datas = [datagen.text_like(rnd.randint(8000, 200000), 500 + k) for k in range(16)]
    hs = [da.gzip_header(filename=b"n" * (1 + k % 8)) for k in range(16)]
    assert {len(h) % 4 for h in hs} == {0, 1, 2, 3}
    outs = ctx.encode_batch_gzip(datas, opts, hs)
    bi = ctx.batch_info()
    assert bi["n_batched"] == 16 and bi["n_single"] == 0  # (the batched kernels took them)
    for k, (d, h) in enumerate(zip(datas, hs)):
        assert outs[k] == ctx.encode_gzip(d, opts, h), (k, len(h) % 4)
        assert outs[k][:len(h)] == h
        assert gzip.decompress(outs[k]) == d


def test_order_and_size_invariance(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    datas = mixed_items()
    hs = named_headers(da, len(datas))
    base = ctx.encode_batch_gzip(datas, opts, hs)
    perm = list(range(len(datas)))
    random.Random(5).shuffle(perm)
    shuffled = ctx.encode_batch_gzip([datas[p] for p in perm], opts, [hs[p] for p in perm])
    assert [shuffled[perm.index(k)] for k in range(len(datas))] == base
    for k in (0, 7, len(datas) - 5, len(datas) - 1):
        assert ctx.encode_batch_gzip([datas[k]], opts, [hs[k]]) == [base[k]]
    h = len(datas) // 2
    assert ctx.encode_batch_gzip(datas[:h], opts, hs[:h]) + ctx.encode_batch_gzip(datas[h:], opts, hs[h:]) == base


def test_routing_is_that_of_the_zlib_batch(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    keys = ("n_batched", "n_single", "n_q1_single", "n_spec_single")
    datas = mixed_items()
    ctx.encode_batch(datas, opts, wrapper=1)
    want = ctx.batch_info()
    outs = ctx.encode_batch_gzip(datas, opts, named_headers(da, len(datas)))
    got = ctx.batch_info()
    assert {k: got[k] for k in keys} == {k: want[k] for k in keys}
    assert got["n_batched"] + got["n_single"] == len(datas) and got["n_batched"] >= 1 and got["n_single"] >= 1
    assert got["in_len"] == sum(map(len, datas)) and got["out_len"] == sum(map(len, outs))
    rnd = random.Random(9)
    texts = [datagen.text_like(rnd.randint(8000, 200000), 100 + k) for k in range(64)]
    outs = ctx.encode_batch_gzip(texts, opts, named_headers(da, 64))
    bi = ctx.batch_info()
    assert bi["n_batched"] == 64 and bi["n_single"] == 0 and bi["sub_batches"] == 1
    assert bi["in_len"] == sum(map(len, texts)) and bi["out_len"] == sum(map(len, outs))
    info = ctx.info()
    assert info["in_len"] == bi["in_len"] and info["out_len"] == bi["out_len"]
    assert ctx.blocks() == []


def test_device_entry_on_a_caller_stream_and_sub_batches(da, ctx):
    opts = da.CompressionOptions(*LV["fast"])
    rnd = random.Random(21)
    datas = [datagen.text_like(rnd.randint(1, 600000), 300 + k) for k in range(12)] + [b""]
    hs = named_headers(da, len(datas))
    ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda")
           for d in datas]
    torch.cuda.synchronize()
    ctx.config(da.Context.CFG_BATCH_BYTES, 1 << 20)
    try:
        s = torch.cuda.Stream()
        outs, lens, st = ctx.encode_batch_device_gzip(ins, options=opts, headers=hs, stream=s.cuda_stream)
    finally:
        ctx.config(da.Context.CFG_BATCH_BYTES, 256 << 20)
    assert st == [0] * len(datas)
    bi = ctx.batch_info()
    assert bi["sub_batches"] >= 2
    for d, h, o, n in zip(datas, hs, outs, lens):
        got = bytes(o[:n].cpu().numpy().tobytes())
        assert got == ctx.encode_gzip(d, opts, h)
        assert gzip.decompress(got) == d


def test_item_errors_and_call_errors(da, ctx):
    L = da.load()
    opts = da.CompressionOptions(*LV["default"])
    t = datagen.text_like(300000, 4)
    datas = [t[:50000], t[50000:120000], t[120000:]]
    hs = [da.gzip_header(filename=b"a"), da.gzip_header(filename=b"bcd", comment=b"second"), da.gzip_header()]
    arr = header_array(da, hs)
    o = opts.to_c(0, 0, 0)  # (the wrapper is taken as 2 whatever it holds)
    good = [ctx.encode_gzip(d, opts, h) for d, h in zip(datas, hs)]
    hlens = [len(h) for h in hs]
    rc, outs, st, _ = raw_batch(da, ctx, datas, o, arr, 3, hlens=hlens)
    assert rc == 0 and st == [0, 0, 0] and outs == good
    # one item a byte short of its bound (which counts its own header)
    caps = [L.mi355_deflate_bound_ex(len(d), 2, n, 0) for d, n in zip(datas, hlens)]
    caps[1] -= 1
    rc, outs, st, lens = raw_batch(da, ctx, datas, o, arr, 3, caps=caps)
    assert rc == E_OUT_TOO_SMALL and st == [0, E_OUT_TOO_SMALL, 0]
    assert lens[1] == caps[1] + 1 == L.mi355_deflate_bound_ex(len(datas[1]), 2, hlens[1], 0)
    assert outs[0] == good[0] and outs[2] == good[2]
    # the call itself: nothing is written to an item
    def refused(o_, hdrs, n_hdrs, want=E_ARG):
        rc_, _, st_, lens_ = raw_batch(da, ctx, datas, o_, hdrs, n_hdrs, hlens=hlens, sentinel=77)
        assert rc_ == want, (rc_, want)
        assert st_ == [77, 77, 77] and lens_ == [0, 0, 0]
    refused(o, arr, 2)                      # neither 0, 1 nor n_items
    refused(o, header_array(da, hs + hs[:1]), 4)
    refused(o, None, 1)                     # NULL hdrs with n_hdrs > 0
    refused(o, None, 3)
    empty = header_array(da, hs)
    empty[2].hdr_len = 0
    refused(o, empty, 3)                    # an entry of length 0
    null = header_array(da, hs)
    null[0].hdr = None
    refused(o, null, 3)                     # an entry with a NULL pointer
    long_h = bytes(0x10000)
    refused(o, header_array(da, [long_h]), 1)   # an entry above 0xFFFF
    refused(opts.to_c(0, 0, 1), arr, 3)     # sync flush
    refused(da.CompressionOptions(128, 2, 1).to_c(0, 0, 0), arr, 3, want=E_UNSUPPORTED)
    assert L.mi355_deflate_encode_batch_gzip(ctx._h, None, 3, C.byref(o), arr, 3) == E_ARG
    assert L.mi355_deflate_encode_batch_gzip(ctx._h, None, 0, C.byref(o), None, 0) == 0
    assert L.mi355_deflate_encode_batch_gzip(ctx._h, None, 0, C.byref(o), arr, 1) == 0
    assert ctx.encode_batch_gzip([], opts) == []
    # the longest header there is goes through
    max_h = da.gzip_header(comment=b"k" * (0xFFFF - 11))
    assert len(max_h) == 0xFFFF
    assert ctx.encode_batch_gzip(datas[:2], opts, max_h) == [ctx.encode_gzip(d, opts, max_h) for d in datas[:2]]
    # the device entry: an unaligned output
    d_in = torch.frombuffer(bytearray(datas[0]), dtype=torch.uint8).cuda()
    d_out = torch.empty(caps[0] + 8, dtype=torch.uint8, device="cuda")
    items = (da.BatchItem * 1)()
    items[0].in_, items[0].in_len, items[0].out, items[0].out_cap = d_in.data_ptr(), len(datas[0]), d_out.data_ptr() + 1, caps[0]
    items[0].status = 77
    assert L.mi355_deflate_encode_batch_device_gzip(ctx._h, items, 1, C.byref(o), arr, 1, None) == E_ARG
    assert items[0].status == 77
    # mi355_deflate_encode_batch keeps refusing wrapper 2
    keep = (C.c_uint8 * 64)()
    items = (da.BatchItem * 1)()
    items[0].in_, items[0].in_len, items[0].out, items[0].out_cap = None, 0, C.cast(keep, C.c_void_p), 64
    items[0].status = 77
    assert L.mi355_deflate_encode_batch(ctx._h, items, 1, C.byref(opts.to_c(2, 0, 0))) == E_ARG
    assert items[0].status == 77
