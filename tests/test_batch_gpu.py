"""The batched encode (mi355_deflate_encode_batch[_device]) on the GPU: every item byte for byte what the one-input call and
the oracle give, whatever the batch around it; the routing counts; per-item errors; the device entry.  pytest -m gpu."""
import ctypes as C
import glob
import os
import random
import sys
import zlib

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
E_ARG, E_OUT_TOO_SMALL, E_REF_PANIC = -1, -2, -5


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


def batch(da, ctx, datas, opts, wrapper=0, compat=0, caps=None):
    """the raw host entry: (rc, outputs, statuses, out_lens)"""
    L = da.load()
    o = opts.to_c(wrapper, compat, 0)
    items = (da.BatchItem * max(len(datas), 1))()
    bufs = []
    for k, d in enumerate(datas):
        cap = L.mi355_deflate_bound_ex(len(d), wrapper, 0, 0) if caps is None else caps[k]
        out = (C.c_uint8 * max(cap, 1))()
        bufs.append((d, out))
        items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
        items[k].in_len = len(d)
        items[k].out = C.cast(out, C.c_void_p)
        items[k].out_cap = cap
    rc = L.mi355_deflate_encode_batch(ctx._h, items, len(datas), C.byref(o))
    outs = [bytes(memoryview(bufs[k][1])[: items[k].out_len]) if items[k].status == 0 else None for k in range(len(datas))]
    return rc, outs, [items[k].status for k in range(len(datas))], [items[k].out_len for k in range(len(datas))]


def single(da, ctx, d, opts, wrapper=0, compat=0):
    try:
        return ctx.encode(d, opts, wrapper=wrapper, compat=compat), 0
    except da.DeflateError as e:
        return None, e.code


@pytest.mark.parametrize("wrapper", [0, 1])
@pytest.mark.parametrize("level", list(LV))
def test_mixed_batch_matches_single_calls_and_oracle(da, ctx, level, wrapper):
    c, l, m = LV[level]
    opts = da.CompressionOptions(c, l, m)
    datas = mixed_items()
    rc, outs, st, _ = batch(da, ctx, datas, opts, wrapper, compat=1)
    first_bad = next((s for s in st if s != 0), 0)
    assert rc == first_bad
    for k, d in enumerate(datas):
        one, code = single(da, ctx, d, opts, wrapper, compat=1)
        assert st[k] == code, (k, len(d))
        if code == 0:
            assert outs[k] == one, "item %d (%d bytes) differs from its one-input call" % (k, len(d))
            assert outs[k] == ob.encode(d, opts=ob.make_opts(c, l, m, wrapper)), "item %d differs from the oracle" % k
            assert (zlib.decompress(outs[k]) if wrapper else zlib.decompress(outs[k], -15)) == d


def test_order_and_size_invariance(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    datas = mixed_items()
    base = ctx.encode_batch(datas, opts)
    perm = list(range(len(datas)))
    random.Random(5).shuffle(perm)
    shuffled = ctx.encode_batch([datas[p] for p in perm], opts)
    assert [shuffled[perm.index(k)] for k in range(len(datas))] == base
    for k in (0, 7, len(datas) - 5, len(datas) - 1):
        assert ctx.encode_batch([datas[k]], opts) == [base[k]]
    h = len(datas) // 2
    assert ctx.encode_batch(datas[:h], opts) + ctx.encode_batch(datas[h:], opts) == base


def test_routing_counts(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    rnd = random.Random(9)
    texts = [datagen.text_like(rnd.randint(8000, 200000), 100 + k) for k in range(64)]
    outs = ctx.encode_batch(texts, opts)
    bi = ctx.batch_info()
    assert bi["n_batched"] == 64 and bi["n_single"] == 0 and bi["n_items"] == 64 and bi["sub_batches"] == 1
    assert bi["in_len"] == sum(map(len, texts)) and bi["out_len"] == sum(map(len, outs))
    info = ctx.info()
    assert info["in_len"] == bi["in_len"] and info["out_len"] == bi["out_len"]
    assert ctx.blocks() == []
    for d, o in zip(texts[:8], outs):
        assert o == ctx.encode(d, opts)
    # the mixed batch: the one-input call of every item says which of them re-warm (Q1) or fall back from the speculative parse
    datas = mixed_items()
    q1 = spec = 0
    for d in datas:
        fresh = da.Context(0)
        fresh.encode(d, opts)
        i = fresh.info()
        fresh.close()
        if 0 < len(d) <= (2 << 20):
            q1 += 1 if i["q1_rewarm"] else 0
            spec += 1 if i["spec_fallback"] else 0
    ctx.encode_batch(datas, opts)
    bi = ctx.batch_info()
    assert bi["n_q1_single"] == q1 and bi["n_spec_single"] == spec
    assert q1 >= 1 and spec >= 1  # (the noise and the zeros take these routes)
    big = sum(1 for d in datas if len(d) > (2 << 20))
    empty = sum(1 for d in datas if not d)
    assert bi["n_single"] == big + empty + q1 + spec
    assert bi["n_batched"] + bi["n_single"] == len(datas)


def test_item_errors_and_call_errors(da, ctx):
    L = da.load()
    opts = da.CompressionOptions(*LV["default"])
    t = datagen.text_like(300000, 4)
    datas = [t[:50000], t[50000:120000], t[120000:]]
    good = [ctx.encode(d, opts) for d in datas]
    caps = [L.mi355_deflate_bound_ex(len(d), 0, 0, 0) for d in datas]
    caps[1] -= 1
    rc, outs, st, lens = batch(da, ctx, datas, opts, caps=caps)
    assert rc == E_OUT_TOO_SMALL and st == [0, E_OUT_TOO_SMALL, 0]
    assert lens[1] == caps[1] + 1
    assert outs[0] == good[0] and outs[2] == good[2]
    with pytest.raises(da.DeflateError, match="item 1"):
        caps2 = list(caps)
        items = (da.BatchItem * 3)()
        for k, d in enumerate(datas):
            items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p)
            items[k].in_len = len(d)
            items[k].out = C.cast((C.c_uint8 * caps2[k])(), C.c_void_p)
            items[k].out_cap = caps2[k]
        rc2 = L.mi355_deflate_encode_batch(ctx._h, items, 3, C.byref(opts.to_c(0, 0, 0)))
        ctx._batch_error(rc2, items)
    # the call itself
    o = opts.to_c(2, 0, 0)
    items = (da.BatchItem * 1)()
    keep = (C.c_uint8 * 64)()
    items[0].in_, items[0].in_len, items[0].out, items[0].out_cap = None, 0, C.cast(keep, C.c_void_p), 64
    items[0].status = 77
    assert L.mi355_deflate_encode_batch(ctx._h, items, 1, C.byref(o)) == E_ARG
    assert items[0].status == 77
    assert L.mi355_deflate_encode_batch(ctx._h, None, 3, C.byref(opts.to_c(0, 0, 0))) == E_ARG
    assert L.mi355_deflate_encode_batch(ctx._h, items, 1, None) == E_ARG
    assert L.mi355_deflate_encode_batch(ctx._h, items, 1, C.byref(opts.to_c(0, 0, 1))) == E_ARG  # sync flush
    assert L.mi355_deflate_encode_batch(ctx._h, None, 0, C.byref(opts.to_c(0, 0, 0))) == 0
    assert ctx.encode_batch([], opts) == []
    assert L.mi355_deflate_encode_batch(ctx._h, items, 1, C.byref(da.CompressionOptions(128, 2, 1).to_c(0, 0, 0))) == -4
    assert items[0].status == 77


def test_device_entry_on_a_caller_stream_and_sub_batches(da, ctx):
    opts = da.CompressionOptions(*LV["fast"])
    rnd = random.Random(21)
    datas = [datagen.text_like(rnd.randint(0, 600000), 300 + k) for k in range(12)] + [b""]
    ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda")
           for d in datas]
    torch.cuda.synchronize()
    ctx.config(da.Context.CFG_BATCH_BYTES, 1 << 20)
    try:
        s = torch.cuda.Stream()
        outs, lens, st = ctx.encode_batch_device(ins, options=opts, wrapper=1, stream=s.cuda_stream)
    finally:
        ctx.config(da.Context.CFG_BATCH_BYTES, 256 << 20)
    assert st == [0] * len(datas)
    bi = ctx.batch_info()
    assert bi["sub_batches"] >= 2
    for d, o, n in zip(datas, outs, lens):
        got = bytes(o[:n].cpu().numpy().tobytes())
        assert got == ctx.encode(d, opts, wrapper=1)
        assert zlib.decompress(got) == d


def test_thousand_random_items(da, ctx):
    opts = da.CompressionOptions(*LV["default"])
    rnd = random.Random(33)
    src = datagen.text_like(1 << 20, 44)
    datas = []
    for k in range(1000):
        n = rnd.randint(0, 150000)
        o = rnd.randint(0, len(src) - n)
        datas.append(src[o:o + n] if k % 3 else datagen.rng_bytes(n, k) if k % 7 == 0 else src[o:o + n][::-1])
    outs = ctx.encode_batch(datas, opts)
    sample = list(range(0, 1000, 1))
    for k in sample[:200]:
        assert outs[k] == ob.encode(datas[k], opts=ob.make_opts(*LV["default"])), k
    for k in sample[200:]:
        assert outs[k] == ctx.encode(datas[k], opts), k
