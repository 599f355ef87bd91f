"""The batched encode at the levels without a hash (rle, huffman_only) on the GPU: the batch's launch set takes the items (kb_nohash
stands where kb_sort and the walk stand at the hashing levels), and every item is byte for byte what its one-input call and the
oracle give -- raw, zlib and gzip, wherever an item lies in memory and whatever lies behind it.  Every check is bit-exact.
pytest -m gpu."""
import glob
import gzip
import os
import random
import re
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
LV = {"rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
SET_MAX = 2 << 20  # the largest item a launch set takes (SMALL_TAIL_SEGS segments of 1 KiB)
MAX_MATCH = 258


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def run_rows():
    """the run generator of tools/batch_bench.py"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import batch_bench
    return batch_bench.run_rows


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


def longest_run(b):
    """the longest run of equal bytes"""
    return max((len(m.group(0)) for m in re.finditer(rb"(.)\1*", b, re.S)), default=0)


def named_headers(da, n):
    """one header per item: file names of varying length (odd and even header lengths), an mtime, a comment now and then"""
    hs = []
    for k in range(n):
        name = b"item-%d" % k + b"x" * (k % 7) + b".txt"
        hs.append(da.gzip_header(filename=name, mtime=1700000000 + k, comment=(b"c" * (k % 5)) if k % 3 == 0 else None))
    return hs


def single(da, ctx, d, opts, wrapper=0, compat=0):
    try:
        return ctx.encode(d, opts, wrapper=wrapper, compat=compat), 0
    except da.DeflateError as e:
        return None, e.code


def no_runs(n, salt=0):
    """n bytes without two equal neighbours"""
    return bytes((i * 7 + (i >> 8) + salt) & 255 for i in range(n))


def runs_of(lengths, n, first=0):
    """n bytes of runs whose lengths cycle through `lengths`; neighbouring runs differ"""
    out = bytearray()
    v, k = first, 0
    while len(out) < n:
        out += bytes([v & 255]) * lengths[k % len(lengths)]
        v += 1 + (k % 3)
        k += 1
    return bytes(out[:n])


# ---- 1. routing: the launch set takes every item (on the parent commit n_batched is 0) ----------------------------------------
@pytest.mark.parametrize("level", list(LV))
def test_routing_everything_is_batched(da, ctx, level):
    opts = da.CompressionOptions(*LV[level])
    rnd = random.Random(9)
    datas = [datagen.text_like(rnd.randint(8000, 200000), 100 + k) for k in range(64)]
    datas += [datagen.rng_bytes(rnd.randint(1, 150000), 700 + k) for k in range(8)]
    # the precondition of "nothing goes single": two parses inside a run of at most 258 bytes both land on its end (rle.rs:46-69)
    assert all(longest_run(d) < MAX_MATCH for d in datas)
    outs = ctx.encode_batch(datas, opts)
    bi = ctx.batch_info()
    print(level, bi)
    assert bi["n_items"] == 72
    assert bi["n_batched"] == 72 and bi["n_single"] == 0 and bi["n_q1_single"] == 0 and bi["n_spec_single"] == 0
    assert bi["sub_batches"] == 1
    assert bi["in_len"] == sum(map(len, datas)) and bi["out_len"] == sum(map(len, outs))
    info = ctx.info()
    assert info["in_len"] == bi["in_len"] and info["out_len"] == bi["out_len"]
    one = da.Context(0)
    try:
        for k, d in enumerate(datas):
            assert outs[k] == one.encode(d, opts), k
            assert one.info()["spec_fallback"] == 0, k
    finally:
        one.close()
    for k in range(0, 72, 9):
        assert outs[k] == ob.encode(datas[k], opts=ob.make_opts(*LV[level])), k


# ---- 2. parity: raw, zlib, gzip with none / one / per-item headers -------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [0, 1])
@pytest.mark.parametrize("level", list(LV))
def test_mixed_batch_matches_single_calls_and_oracle(da, ctx, level, wrapper):
    c, l, m = LV[level]
    opts = da.CompressionOptions(c, l, m)
    datas = mixed_items()
    L = da.load()
    import ctypes as C
    o = opts.to_c(wrapper, 1, 0)
    items = (da.BatchItem * len(datas))()
    bufs = []
    for k, d in enumerate(datas):
        cap = L.mi355_deflate_bound_ex(len(d), wrapper, 0, 0)
        out = (C.c_uint8 * max(cap, 1))()
        bufs.append(out)
        items[k].in_ = C.cast(C.c_char_p(d), C.c_void_p) if d else C.c_void_p(0)
        items[k].in_len = len(d)
        items[k].out = C.cast(out, C.c_void_p)
        items[k].out_cap = cap
    rc = L.mi355_deflate_encode_batch(ctx._h, items, len(datas), C.byref(o))
    st = [items[k].status for k in range(len(datas))]
    assert rc == next((s for s in st if s != 0), 0)
    bi = ctx.batch_info()
    assert bi["n_batched"] >= 1
    for k, d in enumerate(datas):
        one, code = single(da, ctx, d, opts, wrapper, compat=1)
        assert st[k] == code, (k, len(d))
        if code == 0:
            got = bytes(memoryview(bufs[k])[: items[k].out_len])
            assert got == one, "item %d (%d bytes) differs from its one-input call" % (k, len(d))
            assert got == ob.encode(d, opts=ob.make_opts(c, l, m, wrapper)), "item %d differs from the oracle" % k
            assert (zlib.decompress(got) if wrapper else zlib.decompress(got, -15)) == d


@pytest.mark.parametrize("headers_kind", ["blank", "shared", "per_item"])
@pytest.mark.parametrize("level", list(LV))
def test_gzip_batch_matches_single_calls_and_oracle(da, ctx, level, headers_kind):
    c, l, m = LV[level]
    opts = da.CompressionOptions(c, l, m)
    datas = mixed_items()
    per_item = named_headers(da, len(datas))
    assert {len(h) % 2 for h in per_item} == {0, 1} and len({len(h) for h in per_item}) >= 4
    headers = {"blank": None, "shared": da.gzip_header(filename=b"shared-name.bin", mtime=1234567), "per_item": per_item}[headers_kind]
    outs = ctx.encode_batch_gzip(datas, opts, headers)
    bi = ctx.batch_info()
    assert bi["n_batched"] >= 1 and bi["n_batched"] + bi["n_single"] == len(datas)
    for k, d in enumerate(datas):
        h = da.BLANK_GZIP_HEADER if headers is None else headers if isinstance(headers, bytes) else headers[k]
        assert outs[k] == ctx.encode_gzip(d, opts, h), "item %d (%d bytes) differs from its one-input call" % (k, len(d))
        assert outs[k] == ob.encode_gzip(d, h, opts=ob.make_opts(c, l, m, 0)), "item %d differs from the oracle" % k
        assert outs[k][:len(h)] == h
        assert gzip.decompress(outs[k]) == d  # (checks CRC-32 and the length itself)


# ---- 3. mixed routing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", list(LV))
def test_mixed_routing_counts(da, ctx, level):
    opts = da.CompressionOptions(*LV[level])
    datas = mixed_items()
    spec = 0
    for d in datas:
        fresh = da.Context(0)
        fresh.encode(d, opts)
        i = fresh.info()
        fresh.close()
        if 0 < len(d) <= SET_MAX:
            spec += 1 if i["spec_fallback"] else 0
    ctx.encode_batch(datas, opts)
    bi = ctx.batch_info()
    print(level, "spec", spec, bi)
    big = sum(1 for d in datas if len(d) > SET_MAX)
    empty = sum(1 for d in datas if not d)
    assert bi["n_single"] == big + empty + spec
    assert bi["n_spec_single"] == spec and bi["n_q1_single"] == 0
    assert bi["n_batched"] + bi["n_single"] == len(datas)
    if level == "rle":
        assert spec >= 1  # (the megabyte of zeros)
    else:
        assert spec == 0
        # every item of 1 byte to 2 MiB, the 100 000 bytes of noise among them
        assert bi["n_batched"] == sum(1 for d in datas if 0 < len(d) <= SET_MAX)
        assert len(datas[-1]) == 100000


# ---- 4. runs at every seam: the device entry, the items back to back in one allocation at odd byte offsets ---------------------
def seam_items(run_rows):
    cyc = [1, 2, 3, 4, 257, 258, 259, 600]
    items = []
    for n in (1, 2, 3, 4095, 4096, 4097):
        items.append(runs_of([5, 1, 2, 300, 3, 4], n, first=n))
    items.append(runs_of(cyc, 70000))
    items.append(runs_of(cyc[::-1], 33333, first=9))
    # runs across the 4096-position tile boundary: one that ends on it, one that begins on it, short and long ones over it
    items.append(no_runs(3996) + b"A" * 100 + b"B" * 100 + no_runs(4000, 3))            # ends at 4096 / begins at 4096
    items.append(no_runs(4000) + b"C" * 200 + no_runs(3992, 1) + b"D" * 600 + no_runs(50))  # 4000..4200, 8192 inside the 600
    items.append(no_runs(4095) + b"EE" + no_runs(4094, 5) + b"FFF" + no_runs(100))      # 2 and 3 bytes over a tile boundary
    items.append(no_runs(3967) + b"G" * 258 + no_runs(10) + b"H" * 257 + no_runs(3660, 2) + b"I" * 259 + no_runs(7))
    # runs across the 1 KiB segment boundaries
    items.append(no_runs(1000) + b"J" * 100 + no_runs(947, 1) + b"KK" + no_runs(1022, 2) + b"LLL" + no_runs(500) + b"M" * 600 + no_runs(3))
    items.append(no_runs(1023) + b"N" * 258 + no_runs(767, 4) + b"O" * 257 + no_runs(2))
    # a run that ends exactly with its item while the next item begins with the same byte
    items.append(no_runs(700) + b"Z" * 300)
    items.append(b"Z" * 50 + no_runs(900, 1))
    items.append(no_runs(3996, 2) + b"Q" * 100)  # (4096 bytes: the run ends with the item and with its tile)
    items.append(b"Q" * 5 + no_runs(10, 1))
    items.append(b"Q")
    items.append(b"QQ")
    items.append(b"QQQ" + b"R" * 4)
    items.append(run_rows(SET_MAX, 77))
    items.append(runs_of([1, 2, 3, 4, 257, 200, 255, 100], SET_MAX, first=3))
    return items


@pytest.mark.parametrize("wrapper", [0, 1])
@pytest.mark.parametrize("level", list(LV))
def test_runs_at_every_seam_device_entry(da, ctx, run_rows, level, wrapper):
    c, l, m = LV[level]
    opts = da.CompressionOptions(c, l, m)
    datas = seam_items(run_rows)
    assert {len(d) for d in datas} >= {1, 2, 3, 4095, 4096, 4097, SET_MAX}
    lead = b"\x5a"  # (the first item one byte into the allocation)
    big = torch.frombuffer(bytearray(lead + b"".join(datas)), dtype=torch.uint8).cuda()
    ins, off = [], len(lead)
    for d in datas:
        ins.append(big[off:off + len(d)])
        off += len(d)
    ptrs = [x.data_ptr() for x in ins]
    assert all(p + len(d) == q for p, d, q in zip(ptrs, datas, ptrs[1:]))  # back to back
    assert any(p & 1 for p in ptrs) and sum(1 for p in ptrs if p & 15) >= len(ptrs) // 2  # (the unaligned staging of k_rle)
    torch.cuda.synchronize()
    outs, lens, st = ctx.encode_batch_device(ins, options=opts, wrapper=wrapper, compat=1)
    bi = ctx.batch_info()
    print(level, wrapper, bi)
    assert st == [0] * len(datas)
    # every item whose runs are shorter than 258 bytes re-joins, so the set keeps it
    may_fall_back = sum(1 for d in datas if longest_run(d) >= MAX_MATCH)
    assert bi["n_single"] == bi["n_spec_single"] <= may_fall_back and bi["n_batched"] + bi["n_single"] == len(datas)
    if level == "huffman_only":
        assert bi["n_single"] == 0
    for k, (d, o, n) in enumerate(zip(datas, outs, lens)):
        got = bytes(o[:n].cpu().numpy().tobytes())
        assert got == ob.encode(d, opts=ob.make_opts(c, l, m, wrapper)), "item %d (%d bytes) differs from the oracle" % (k, len(d))
        assert got == ctx.encode(d, opts, wrapper=wrapper, compat=1), "item %d (%d bytes) differs from its one-input call" % (k, len(d))
    assert bytes(big.cpu().numpy().tobytes()) == lead + b"".join(datas)


# ---- 5. invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", list(LV))
def test_order_and_size_invariance(da, ctx, run_rows, level):
    opts = da.CompressionOptions(*LV[level])
    datas = mixed_items() + [run_rows(50000, 5), run_rows(4097, 6)]
    base = ctx.encode_batch(datas, opts)
    perm = list(range(len(datas)))
    random.Random(5).shuffle(perm)
    shuffled = ctx.encode_batch([datas[p] for p in perm], opts)
    assert [shuffled[perm.index(k)] for k in range(len(datas))] == base
    for k in (0, 1, 7, len(datas) - 5, len(datas) - 3, len(datas) - 1):
        assert ctx.encode_batch([datas[k]], opts) == [base[k]]
    h = len(datas) // 2
    assert ctx.encode_batch(datas[:h], opts) + ctx.encode_batch(datas[h:], opts) == base


@pytest.mark.parametrize("level", list(LV))
def test_sub_batches_on_a_caller_stream(da, ctx, run_rows, level):
    opts = da.CompressionOptions(*LV[level])
    rnd = random.Random(21)
    datas = [datagen.text_like(rnd.randint(0, 600000), 300 + k) for k in range(8)] + [b""]
    datas += [run_rows(rnd.randint(1, 600000), 40 + k) for k in range(4)]
    ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda")
           for d in datas]
    torch.cuda.synchronize()
    outs0, lens0, st0 = ctx.encode_batch_device(ins, options=opts, wrapper=1)
    assert ctx.batch_info()["sub_batches"] == 1
    whole = [bytes(o[:n].cpu().numpy().tobytes()) for o, n in zip(outs0, lens0)]
    ctx.config(da.Context.CFG_BATCH_BYTES, 1 << 20)
    try:
        s = torch.cuda.Stream()
        outs, lens, st = ctx.encode_batch_device(ins, options=opts, wrapper=1, stream=s.cuda_stream)
        bi = ctx.batch_info()
    finally:
        ctx.config(da.Context.CFG_BATCH_BYTES, 256 << 20)
    assert st == [0] * len(datas) and st0 == st
    assert bi["sub_batches"] >= 2 and bi["n_batched"] == sum(1 for d in datas if d) and bi["n_single"] == sum(1 for d in datas if not d)
    for d, o, n, w in zip(datas, outs, lens, whole):
        got = bytes(o[:n].cpu().numpy().tobytes())
        assert got == w
        assert got == ctx.encode(d, opts, wrapper=1)
        assert zlib.decompress(got) == d


# ---- 6. a thousand items at rle ------------------------------------------------------------------------------------------------
def test_thousand_items_rle(da, ctx, run_rows):
    opts = da.CompressionOptions(*LV["rle"])
    rnd = random.Random(33)
    text = datagen.text_like(1 << 20, 44)
    runs = run_rows(1 << 20, 45)
    datas = []
    for k in range(1000):
        n = rnd.randint(0, 150000)
        o = rnd.randint(0, (1 << 20) - n)
        datas.append(datagen.rng_bytes(n, k) if k % 7 == 0 else runs[o:o + n] if k % 2 else text[o:o + n])
    outs = ctx.encode_batch(datas, opts)
    bi = ctx.batch_info()
    print(bi)
    # (runs of at most 200 bytes, text, noise: nothing falls back; the empty items go singly)
    assert bi["n_single"] == sum(1 for d in datas if not d) and bi["n_batched"] + bi["n_single"] == 1000
    for k in range(200):
        assert outs[k] == ob.encode(datas[k], opts=ob.make_opts(*LV["rle"])), k
    for k in range(200, 1000):
        assert outs[k] == ctx.encode(datas[k], opts), k


def test_steps_by_their_own_kernel_give_the_same_bytes(da, ctx, run_rows):
    """MI355_CFG_STEPS_IN_EMIT = 0: at huffman_only the set launches kb_adv and the <false> forms; at rle nothing changes"""
    datas = [datagen.text_like(70000, 1), run_rows(40000, 2), datagen.rng_bytes(5000, 3), b"a", no_runs(4097)]
    for level in LV:
        opts = da.CompressionOptions(*LV[level])
        base = ctx.encode_batch(datas, opts)
        ctx.config(da.Context.CFG_STEPS_IN_EMIT, 0)
        try:
            other = ctx.encode_batch(datas, opts)
            bi = ctx.batch_info()
        finally:
            ctx.config(da.Context.CFG_STEPS_IN_EMIT, 1)
        assert other == base and bi["n_batched"] == len(datas)
        assert base == [ob.encode(d, opts=ob.make_opts(*LV[level])) for d in datas]
