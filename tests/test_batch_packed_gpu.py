"""The packed batch (mi355_deflate_encode_batch_packed[_device]) on the GPU: every item's region of the one arena holds byte
for byte what the one-input call gives for that item alone (and, for a subset, the oracle); the regions are aligned, disjoint
and dense with zero pad bytes; the scan behind the offsets at its chunk boundaries; order, batch size and launch-set cuts do
not matter; an arena smaller than the bound, down to one byte short of what is needed; the device table; host entry against
device entry; the errors of the call; an item on which the reference panics.  pytest -m gpu."""
import ctypes as C
import glob
import os
import random
import sys

import numpy as np
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
E_ARG, E_OUT_TOO_SMALL, E_UNSUPPORTED, E_REF_PANIC = -1, -2, -4, -5
GUARD, FILL = 64, 0xA5
ENTRY = np.dtype([("off", "<u8"), ("len", "<u8"), ("status", "<i4"), ("reserved", "<u4")])
PLACE_T = 1024  # items per round of kb_place's scan (deflate_batch.inc)


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


def align_up(v, a):
    return (v + a - 1) // a * a


def fixtures():
    out = []
    for p in sorted(glob.glob(os.path.join(FIX, "*")) + glob.glob(os.path.join(FIX, "afl", "**", "*"), recursive=True)):
        if os.path.isfile(p):
            out.append(open(p, "rb").read())
    return out


_ITEMS = {}


def parity_items():
    """tiny items, texts, the reference fixtures; in the middle of the list the four that leave the launch sets: noise (Q1),
    zeros (speculative fallback), an empty item and one of 2 MiB + 1"""
    if "parity" not in _ITEMS:
        rnd = random.Random(17)
        texts = [datagen.text_like(rnd.randint(8000, 200000), 500 + k) for k in range(6)]
        big = datagen.text_like((2 << 20) + 1, 12)
        special = [datagen.rng_bytes(100000, 3), bytes(1 << 20), b"", big]
        _ITEMS["parity"] = [b"a", b"ab", b"abc", b"abcd", b"abcde"] + texts[:3] + special + texts[3:] + fixtures()
    return _ITEMS["parity"]


def text_items():
    if "text" not in _ITEMS:
        rnd = random.Random(23)
        _ITEMS["text"] = [datagen.text_like(rnd.randint(8000, 200000), 700 + k) for k in range(12)]
    return _ITEMS["text"]


def named_headers(da, n):
    """one header per item: file names of varying length (odd and even header lengths, so the streams start on every byte of
    a word), an mtime, a comment now and then -- the recipe of test_batch_gzip_gpu.py"""
    hs = []
    for k in range(n):
        name = b"item-%d" % k + b"x" * (k % 7) + b".txt"
        hs.append(da.gzip_header(filename=name, mtime=1700000000 + k, comment=(b"c" * (k % 5)) if k % 3 == 0 else None))
    return hs


_SINGLE = {}


def single(da, ctx, d, lv, wrapper, header=None, compat=0):
    """(bytes or None, status) of the one-input call, computed once per input and setting"""
    key = (d, lv, wrapper, header, compat)
    if key not in _SINGLE:
        opts = da.CompressionOptions(*lv)
        try:
            if wrapper == 2:
                _SINGLE[key] = (ctx.encode_gzip(d, opts, header, compat=compat), 0)
            else:
                _SINGLE[key] = (ctx.encode(d, opts, wrapper=wrapper, compat=compat), 0)
        except da.DeflateError as e:
            _SINGLE[key] = (None, e.code)
    return _SINGLE[key]


def header_of(da, headers, k):
    if headers is None:
        return da.BLANK_GZIP_HEADER
    return headers if isinstance(headers, bytes) else headers[k]


def expected(da, ctx, datas, lv, wrapper, headers=None, compat=0):
    return [single(da, ctx, d, lv, wrapper, header_of(da, headers, k) if wrapper == 2 else None, compat) for k, d in enumerate(datas)]


def run_host(da, ctx, datas, lv, wrapper=0, headers=None, align=4, cap=None, compat=0):
    """the host entry into an arena with GUARD bytes of FILL behind arena_cap: (PackedResult, the arena's bytes with the guard)"""
    if cap is None:
        cap = da.packed_bound([len(d) for d in datas], wrapper, headers, align)
    arena = (C.c_uint8 * (cap + GUARD))()
    C.memset(arena, FILL, cap + GUARD)
    res = ctx.encode_batch_packed(datas, da.CompressionOptions(*lv), wrapper=wrapper, headers=headers, align=align, compat=compat,
                                  arena=arena, arena_cap=cap, check=False)
    raw = bytes(arena)
    assert raw[cap:] == bytes([FILL]) * GUARD, "host entry wrote behind arena_cap"
    return res, raw


def to_device(datas):
    ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() if d else torch.empty(0, dtype=torch.uint8, device="cuda")
           for d in datas]
    torch.cuda.synchronize()
    return ins


def run_device(da, ctx, ins, lv, wrapper=0, headers=None, align=4, cap=None, compat=0, stream=0):
    """the device entry into an arena tensor with GUARD bytes of FILL behind arena_cap, with a table:
    (PackedResult, the arena's bytes with the guard, the table as a structured array)"""
    lens = [int(t.numel()) for t in ins]
    if cap is None:
        cap = da.packed_bound(lens, wrapper, headers, align)
    arena = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    table = torch.full((24 * max(len(ins), 1),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = ctx.encode_batch_packed_device(ins, arena, da.CompressionOptions(*lv), wrapper=wrapper, headers=headers, align=align,
                                         compat=compat, arena_cap=cap, table=table, stream=stream, check=False)
    raw = arena.cpu().numpy().tobytes()
    assert raw[cap:] == bytes([FILL]) * GUARD, "device entry wrote behind arena_cap"
    tab = np.frombuffer(table.cpu().numpy().tobytes(), dtype=ENTRY)[: len(ins)]
    return res, raw, tab


def check_layout(res, raw, want, align, cap):
    """the contract's layout for what fitted: bytes, alignment, disjoint and dense regions, zero pads, arena_used"""
    assert len(res.entries) == len(want)
    regions = []
    for k, ((off, ln), st, (exp, code)) in enumerate(zip(res.entries, res.statuses, want)):
        if st == E_OUT_TOO_SMALL and code == 0:
            assert off is None and ln == len(exp), k  # (its exact length all the same)
            continue
        assert st == code, (k, st, code)
        if code != 0:
            assert off is None and ln == 0, k
            continue
        assert ln == len(exp), (k, ln, len(exp))
        assert off is not None and off % align == 0, (k, off)
        assert off + align_up(ln, align) <= cap, k
        assert raw[off:off + ln] == exp, "item %d (%d bytes in the arena at %d) differs from its one-input call" % (k, ln, off)
        assert raw[off + ln:off + align_up(ln, align)] == bytes(align_up(ln, align) - ln), "item %d: pad bytes" % k
        regions.append((off, align_up(ln, align)))
    regions.sort()
    end = 0
    for off, size in regions:  # zero-length regions cannot occur: every stream has a byte
        assert off >= end, "regions overlap at %d" % off
        end = off + size
    return regions, end


def check_complete(res, raw, want, align, cap):
    """... of a call in which every OK item fitted: dense from 0, arena_used the end of the last region"""
    regions, end = check_layout(res, raw, want, align, cap)
    at = 0
    for off, size in regions:
        assert off == at, "a gap before %d" % off
        at += size
    assert res.used == at == sum(align_up(len(e), align) for e, code in want if code == 0)
    codes = [code for _, code in want]
    assert res.rc == next((c for c in codes if c != 0), 0)
    assert res.statuses == codes


# ---- 1. parity and layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [0, 1, 2])
@pytest.mark.parametrize("level", list(LV))
def test_parity_and_layout(da, ctx, level, wrapper):
    lv = LV[level]
    datas = parity_items()
    headers = named_headers(da, len(datas)) if wrapper == 2 else None
    if wrapper == 2:
        assert {len(h) % 2 for h in headers} == {0, 1}
    want = expected(da, ctx, datas, lv, wrapper, headers)
    assert all(code == 0 for _, code in want)
    assert {len(e) % 4 for e, _ in want} == {0, 1, 2, 3}, "the streams' lengths must cover every residue mod 4"
    c, l, m = lv
    for k in list(range(8)) + [len(datas) - 1]:  # the oracle for a subset (the small ones)
        if wrapper == 2:
            assert want[k][0] == ob.encode_gzip(datas[k], headers[k], opts=ob.make_opts(c, l, m, 0)), k
        else:
            assert want[k][0] == ob.encode(datas[k], opts=ob.make_opts(c, l, m, wrapper)), k
    # the routing of the existing entry on the same items
    opts = da.CompressionOptions(*lv)
    if wrapper == 2:
        ctx.encode_batch_gzip(datas, opts, headers)
    else:
        ctx.encode_batch(datas, opts, wrapper=wrapper)
    routing = ctx.batch_info()
    assert routing["n_single"] >= 2  # (the empty item and the long one at every level)
    for align in (4, 8, 256):
        cap = da.packed_bound([len(d) for d in datas], wrapper, headers, align)
        res, raw = run_host(da, ctx, datas, lv, wrapper, headers, align)
        check_complete(res, raw, want, align, cap)
        bi = ctx.batch_info()
        for f in ("n_items", "in_len", "out_len", "n_batched", "n_single", "n_q1_single", "n_spec_single", "sub_batches"):
            assert bi[f] == routing[f], (f, align)
        info = ctx.info()
        assert info["in_len"] == bi["in_len"] and info["out_len"] == bi["out_len"]
        assert ctx.blocks() == []


def test_blank_and_shared_gzip_headers_and_the_python_surface(da, ctx):
    lv = LV["default"]
    datas = parity_items()[:10]
    for headers in (None, da.gzip_header(filename=b"shared-name.bin", mtime=1234567)):
        want = expected(da, ctx, datas, lv, 2, headers)
        res, raw = run_host(da, ctx, datas, lv, 2, headers, 8)
        check_complete(res, raw, want, 8, len(raw) - GUARD)
    # the plain return value: (arena, [(off, len), ...]); an exception for a failing item
    arena, entries = ctx.encode_batch_packed(datas, da.CompressionOptions(*lv), wrapper=1, align=8)
    want = expected(da, ctx, datas, lv, 1)
    assert [bytes(arena[o:o + n]) for o, n in entries] == [e for e, _ in want]
    assert len(arena) == sum(align_up(n, 8) for _, n in entries)
    assert da.deflate_bytes_batch_packed(datas[:3], ctx)[1] == [(o, n) for o, n in ctx.encode_batch_packed(datas[:3])[1]]
    with pytest.raises(da.DeflateError, match="item"):
        ctx.encode_batch_packed(datas, da.CompressionOptions(*lv), arena_cap=64)


# ---- 2. the scan's boundaries ----------------------------------------------------------------------------------------------
def scan_counts():
    counts = {1, 2, 63, 64, 65, 1023, 1024, 1025, 4100}
    # whatever a round of kb_place takes: one below, at and above one and two rounds -- in items of the launch set, of which
    # a batch of n holds n - ceil(n / 3) (every third item is empty and goes the other way; a stray item whose speculative parse
    # fails moves a count by one, which the neighbouring counts cover)
    for k in (PLACE_T - 1, PLACE_T, PLACE_T + 1, 2 * PLACE_T - 1, 2 * PLACE_T, 2 * PLACE_T + 1):
        counts.add(next(n for n in range(k, 2 * k + 3) if n - (n + 2) // 3 == k))
    return sorted(counts)


def scan_pool(n):
    if "scan" not in _ITEMS:
        src = datagen.text_like(1 << 16, 91)
        _ITEMS["scan"] = [src[257 * j:257 * j + 40 + j] for j in range(261)]  # 40 .. 300 bytes of text
    pool = _ITEMS["scan"]
    return [b"" if k % 3 == 0 else pool[(k * 7) % 261] for k in range(n)]


@pytest.mark.parametrize("n", scan_counts())
def test_scan_boundaries(da, ctx, n):
    lv = LV["default"]
    datas = scan_pool(n)
    want = expected(da, ctx, datas, lv, 0)
    align = 8 if n % 2 else 4
    res, raw = run_host(da, ctx, datas, lv, 0, None, align)
    check_complete(res, raw, want, align, len(raw) - GUARD)
    bi = ctx.batch_info()
    ctx.encode_batch(datas, da.CompressionOptions(*lv))  # the routing of the existing entry
    routing = ctx.batch_info()
    assert (bi["n_single"], bi["n_batched"]) == (routing["n_single"], routing["n_batched"])
    # (the empty ones, and now and then a short text whose speculative parse the one-input path does again)
    assert (n + 2) // 3 <= bi["n_single"] <= (n + 2) // 3 + n // 32 + 1 and bi["n_batched"] + bi["n_single"] == n


# ---- 3. order and cuts -----------------------------------------------------------------------------------------------------
def test_order_and_cut_independence(da, ctx):
    lv = LV["default"]
    datas = parity_items()[:16]
    want = expected(da, ctx, datas, lv, 1)
    perm = list(range(len(datas)))
    random.Random(5).shuffle(perm)
    res, raw = run_host(da, ctx, [datas[p] for p in perm], lv, 1, None, 8)
    check_complete(res, raw, [want[p] for p in perm], 8, len(raw) - GUARD)
    for k in (0, 5, 8, 9, 15):
        res, raw = run_host(da, ctx, [datas[k]], lv, 1, None, 4)
        check_complete(res, raw, [want[k]], 4, len(raw) - GUARD)
    h = len(datas) // 2
    for part, w in ((datas[:h], want[:h]), (datas[h:], want[h:])):
        res, raw = run_host(da, ctx, part, lv, 1, None, 4)
        check_complete(res, raw, w, 4, len(raw) - GUARD)


def test_launch_set_cuts_carry_the_tail(da, ctx):
    lv = LV["fast"]
    src = datagen.text_like(3 << 20, 31)
    rnd = random.Random(41)
    datas, at = [], 0
    while at < len(src):
        n = rnd.randint(60000, 200000)
        datas.append(src[at:at + n])
        at += n
    datas.insert(3, b"")
    want = expected(da, ctx, datas, lv, 1)
    ins = to_device(datas)
    ctx.config(da.Context.CFG_BATCH_BYTES, 1 << 20)
    try:
        res, raw = run_host(da, ctx, datas, lv, 1, None, 8)
        bi = ctx.batch_info()
        s = torch.cuda.Stream()
        dres, draw, tab = run_device(da, ctx, ins, lv, 1, None, 8, stream=s.cuda_stream)
        dbi = ctx.batch_info()
    finally:
        ctx.config(da.Context.CFG_BATCH_BYTES, 256 << 20)
    assert bi["sub_batches"] >= 2 and dbi["sub_batches"] == bi["sub_batches"]
    check_complete(res, raw, want, 8, len(raw) - GUARD)
    check_complete(dres, draw, want, 8, len(draw) - GUARD)
    assert dres.entries == res.entries


# ---- 4. a small arena ------------------------------------------------------------------------------------------------------
def small_items():
    """the texts with one item of the one-input path (noise: Q1) in the middle, its region behind the launch set's"""
    t = text_items()
    return t[:6] + [datagen.rng_bytes(100000, 3)] + t[6:]


def check_table(tab, res, full):
    """the device table says what the items say; where an item has no place, the offset it was assigned (those of the call with
    room for all)"""
    for k, ((off, ln), st) in enumerate(zip(res.entries, res.statuses)):
        assert int(tab["len"][k]) == ln and int(tab["status"][k]) == st and int(tab["reserved"][k]) == 0, k
        if st == 0:
            assert int(tab["off"][k]) == off, k
        elif st == E_OUT_TOO_SMALL:
            assert int(tab["off"][k]) == full.entries[k][0], k


def test_small_arena(da, ctx):
    lv, align = LV["default"], 8
    texts = text_items()
    twant = expected(da, ctx, texts, lv, 0)
    half = sum(map(len, texts)) // 2
    assert half < da.packed_bound([len(d) for d in texts], 0, None, align) // 2
    res, raw = run_host(da, ctx, texts, lv, 0, None, align, cap=half)
    check_complete(res, raw, twant, align, half)
    # one byte short of what the launch set alone needs: its last item, and only that one, is left out by kb_place
    tins = to_device(texts)
    for r, b in (run_host(da, ctx, texts, lv, 0, None, align, cap=res.used - 1),
                 run_device(da, ctx, tins, lv, 0, None, align, cap=res.used - 1)[:2]):
        assert r.rc == E_OUT_TOO_SMALL and r.used == res.used
        assert r.statuses == [0] * (len(texts) - 1) + [E_OUT_TOO_SMALL] and r.entries[:-1] == res.entries[:-1]
        assert r.entries[-1] == (None, len(twant[-1][0]))
        check_layout(r, b, twant, align, res.used - 1)

    datas = small_items()
    ins = to_device(datas)
    want = expected(da, ctx, datas, lv, 0)
    full, fraw = run_host(da, ctx, datas, lv, 0, None, align)
    check_complete(full, fraw, want, align, len(fraw) - GUARD)
    needed = full.used
    mid = full.entries[5][0] + 11  # a cut inside the region of an item in the middle of the launch set
    for cap in (needed - 1, mid, 0):
        unfit = [k for k, (off, ln) in enumerate(full.entries) if off + align_up(ln, align) > cap]
        assert unfit and (cap != mid or len(unfit) > 3)
        hres, hraw = run_host(da, ctx, datas, lv, 0, None, align, cap=cap)
        dres, draw, tab = run_device(da, ctx, ins, lv, 0, None, align, cap=cap)
        for r, b in ((hres, hraw), (dres, draw)):
            assert r.rc == E_OUT_TOO_SMALL and r.used == needed
            assert [k for k, s in enumerate(r.statuses) if s != 0] == unfit
            assert [r.statuses[k] for k in unfit] == [E_OUT_TOO_SMALL] * len(unfit)
            assert [ln for _, ln in r.entries] == [len(e) for e, _ in want]  # every out_len exact
            check_layout(r, b, want, align, cap)
            for k in range(len(datas)):  # what fits lies where it lies with room for all
                if k not in unfit:
                    assert r.entries[k] == full.entries[k]
        check_table(tab, dres, full)
    hres, hraw = run_host(da, ctx, datas, lv, 0, None, align, cap=needed)
    check_complete(hres, hraw, want, align, needed)
    dres, draw, tab = run_device(da, ctx, ins, lv, 0, None, align, cap=needed)
    check_complete(dres, draw, want, align, needed)
    check_table(tab, dres, full)


# ---- 5. and 6. the device table; host against device -------------------------------------------------------------------------
@pytest.mark.parametrize("wrapper", [0, 2])
def test_device_table_and_host_against_device(da, ctx, wrapper):
    lv, align = LV["default"], 256
    datas = parity_items()
    headers = named_headers(da, len(datas)) if wrapper == 2 else None
    want = expected(da, ctx, datas, lv, wrapper, headers)
    ins = to_device(datas)
    hres, hraw = run_host(da, ctx, datas, lv, wrapper, headers, align)
    dres, draw, tab = run_device(da, ctx, ins, lv, wrapper, headers, align)
    check_complete(dres, draw, want, align, len(draw) - GUARD)
    check_table(tab, dres, dres)
    assert [int(x) for x in tab["off"]] == [off for off, _ in dres.entries]  # (the single-path items among them)
    assert dres.entries == hres.entries and dres.statuses == hres.statuses and dres.used == hres.used and dres.rc == hres.rc
    assert draw[:dres.used] == hraw[:hres.used]
    # without a table, and an arena made by the call
    r = ctx.encode_batch_packed_device(ins, None, da.CompressionOptions(*lv), wrapper=wrapper, headers=headers, align=align)
    assert r.entries == dres.entries and r.arena[:r.used].cpu().numpy().tobytes() == draw[:dres.used]


# ---- 7. the errors of the call ------------------------------------------------------------------------------------------------
def test_call_errors(da, ctx):
    L = da.load()
    opts = da.CompressionOptions(*LV["default"])
    d = datagen.text_like(5000, 2)
    dt = to_device([d])[0]
    cap = da.packed_bound([len(d)], 0, None, 4096)
    hdr = da.gzip_header(filename=b"a.txt")
    harr = (da.GzipHeader * 2)()
    for k in range(2):
        harr[k].hdr, harr[k].hdr_len = hdr, len(hdr)

    def call(device, o=None, align=4, n_items=1, arena="own", hdrs=None, n_hdrs=0):
        """(rc, the item and arena_used untouched, no arena byte written)"""
        items = (da.BatchItem * 2)()
        for k in range(2):
            items[k].in_ = C.c_void_p(dt.data_ptr()) if device else C.cast(C.c_char_p(d), C.c_void_p)
            items[k].in_len = len(d)
            items[k].out, items[k].out_cap, items[k].out_len, items[k].status = 0x1234, 5, 6, 77
        used = C.c_size_t(4242)
        o = o if o is not None else opts.to_c(0, 0, 0)
        if device:
            buf = torch.full((2 * cap + 8192,), FILL, dtype=torch.uint8, device="cuda")
            base = (buf.data_ptr() + 4095) // 4096 * 4096
            ptr = {"own": base, "null": 0, "misaligned": base + 4}[arena]
            torch.cuda.synchronize()
            rc = L.mi355_deflate_encode_batch_packed_device(ctx._h, items, n_items, C.byref(o), hdrs, n_hdrs, C.c_void_p(ptr), 2 * cap,
                                                            align, None, C.byref(used), None)
            clean = bool((buf == FILL).all().item())
        else:
            buf = (C.c_uint8 * (2 * cap))()
            C.memset(buf, FILL, 2 * cap)
            ptr = C.cast(buf, C.c_void_p) if arena == "own" else None
            rc = L.mi355_deflate_encode_batch_packed(ctx._h, items, n_items, C.byref(o), hdrs, n_hdrs, ptr, 2 * cap, align, C.byref(used))
            clean = bytes(buf) == bytes([FILL]) * (2 * cap)
        untouched = all((items[k].out, items[k].out_cap, items[k].out_len, items[k].status) == (0x1234, 5, 6, 77) for k in range(2))
        return rc, untouched and used.value == 4242 and clean

    for device in (False, True):
        for align in (3, 6, 8192, 2, 1):
            assert call(device, align=align) == (E_ARG, True), (device, align)
        assert call(device, arena="null") == (E_ARG, True)
        assert call(device, o=opts.to_c(0, 0, 1)) == (E_ARG, True)  # a sync flush
        assert call(device, o=opts.to_c(3, 0, 0)) == (E_ARG, True)  # no such wrapper
        assert call(device, o=opts.to_c(2, 0, 0), n_items=2, hdrs=harr, n_hdrs=3) == (E_ARG, True)
        assert call(device, o=opts.to_c(2, 0, 0), n_items=1, hdrs=None, n_hdrs=1) == (E_ARG, True)
        assert call(device, o=da.CompressionOptions(128, 2, 1).to_c(0, 0, 0)) == (E_UNSUPPORTED, True)
        # (hdrs are not read unless the wrapper is 2; align 0 is 4; 4096 is the largest)
        assert call(device, o=opts.to_c(1, 0, 0), hdrs=None, n_hdrs=7)[0] == 0
        assert call(device, align=0)[0] == 0 and call(device, align=4096)[0] == 0
    assert call(True, align=8, arena="misaligned") == (E_ARG, True)
    assert call(True, align=4, arena="misaligned")[0] == 0
    # an empty batch
    used = C.c_size_t(4242)
    assert L.mi355_deflate_encode_batch_packed(ctx._h, None, 0, C.byref(opts.to_c(0, 0, 0)), None, 0, None, 0, 4, C.byref(used)) == 0
    assert used.value == 0
    used = C.c_size_t(4242)
    assert L.mi355_deflate_encode_batch_packed_device(ctx._h, None, 0, C.byref(opts.to_c(0, 0, 0)), None, 0, None, 0, 4, None,
                                                      C.byref(used), None) == 0
    assert used.value == 0
    assert ctx.encode_batch_packed([], opts) == (bytearray(), [])
    assert L.mi355_deflate_encode_batch_packed(ctx._h, None, 2, C.byref(opts.to_c(0, 0, 0)), None, 0, None, 0, 4, None) == E_ARG
    assert L.mi355_deflate_encode_batch_packed(ctx._h, None, 0, None, None, 0, None, 0, 4, None) == E_ARG


# ---- 8. an item on which the reference panics -----------------------------------------------------------------------------------
def test_ref_panic_takes_no_bytes(da, ctx):
    from test_stages_vs_oracle import q13_case
    lv = LV["default"]
    bad = q13_case(1, total=120000)  # test_q13_modes' recipe, cut short: the slid window reaches beyond the input (A.4 Q13)
    with pytest.raises(ob.RefPanic):
        ob.encode(bad, level=ob.DEFAULT)
    t = text_items()
    datas = [t[0], bad, t[1], b"abc", t[2]]
    want = expected(da, ctx, datas, lv, 0, compat=da.COMPAT_Q13)
    assert [code for _, code in want] == [0, E_REF_PANIC, 0, 0, 0]
    res, raw = run_host(da, ctx, datas, lv, 0, None, 8, compat=da.COMPAT_Q13)
    check_complete(res, raw, want, 8, len(raw) - GUARD)
    assert res.rc == E_REF_PANIC and res.entries[1] == (None, 0)
    dres, draw, tab = run_device(da, ctx, to_device(datas), lv, 0, None, 8, compat=da.COMPAT_Q13)
    check_complete(dres, draw, want, 8, len(draw) - GUARD)
    check_table(tab, dres, dres)
    assert int(tab["status"][1]) == E_REF_PANIC and int(tab["len"][1]) == 0
    # without the compat bit the same input is an item like the others
    want0 = expected(da, ctx, datas, lv, 0)
    res, raw = run_host(da, ctx, datas, lv, 0, None, 8)
    check_complete(res, raw, want0, 8, len(raw) - GUARD)
