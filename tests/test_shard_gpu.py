"""The per-rank phases of the sharded (P1) encode on the GPU -- mi355_shard_begin / _spec / _exit_table / _emit / _blocks_ex / _pack
with k_cover, k_shard_bounds, k_shard_costs and k_seg_exit / k_level_up / k_level_down / k_emit<0> over a range, and
mi355_plan_blocks -- on the inputs and cuts of tests/shard_cases.py: seams with the rank before left 0 to 258 and, by the levels'
largest steps, 286 and 382 bytes into the next, token counts that are 0 and +-1 mod 31744 at a cut, ranks that own nothing, tails
made of several heads, last ranges that a match jumps over (one of them the owner of an empty final block), ranges of 1, 16, 17, 256
and 257 segments on periodic data, every parse_lo and look-ahead the C ABI allows and the drivers never use, the Q13 block cut in
three ways, Stored blocks that begin one token in front of a cut.  tests/test_shard_cases.py asserts on the CPU that every case
forces what its name says, so a failure here points at what only the GPU runs.

The test drives the phases itself, on eight contexts, and holds every exchange to the model, not only the stitched stream: where a
rank says its speculation held, its entry and exit; every entry of every exit table; the entries; token counts and the tokens
themselves; the number of blocks a rank owns, their bytes and Q13 flags; the plan against the oracle's block table; and of the
packed bytes of every rank that no bit is set outside the bit range of its own blocks -- a stray bit that a neighbour's 1 would hide
in the OR-stitched stream.  Then the stitched whole, and shard.encode_p1_virtual on the same cuts.  pytest -m gpu."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import oracle_binding as ob
import shard_cases as sc

shard = sc.shard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctxs(da):
    cs = [da.Context(0) for _ in range(sc.MAX_RANKS)]
    yield cs
    for c in cs:
        c.close()


def _bits(b):
    return np.unpackbits(np.frombuffer(bytes(b), dtype=np.uint8), bitorder="little")


def _words(ptr, n):
    """n token words from the device"""
    if not n:
        return np.zeros(0, dtype=np.int64)
    t = torch.empty(n, dtype=torch.int32, device="cuda:0")
    shard.ctypes_copy_d2d(t.data_ptr(), ptr, 4 * n)
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _same_tokens(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        i = int(np.argmax(got != want))
        raise AssertionError("%s: token %d is %#x (length %d, distance %d), the oracle's is %#x" % (what, i, got[i], (got[i] & 0xFF) + 3, got[i] >> 16, want[i]))


def drive(da, ctxs, c, compat, reemit=False):
    """every phase of every rank of a case, each result held to the model; -> the stitched stream"""
    m = sc.model_of(c)
    lay, world, data, name = m["lay"], m["world"], c["data"], c["name"]
    total = len(data)
    opts = da.CompressionOptions(*c["opts"])
    bufs, shards, keep = [], [], []
    try:
        for r, L in enumerate(lay):
            t = torch.frombuffer(bytearray(data[L["g_lo"]:L["g_hi"]]) + bytearray(16), dtype=torch.uint8).to("cuda:0")
            bufs.append(t)
            shards.append(da.Shard(ctxs[r], t.data_ptr(), L["g_hi"] - L["g_lo"], L["lo"], L["hi"], L["g_lo"], total, opts, compat))
        # ---- entries
        specs = [s.spec() for s in shards]
        for r, (held, e, x) in enumerate(specs):
            if held:
                assert (lay[r]["g_lo"] + e, lay[r]["g_lo"] + x) == (m["spec_entry"][r], m["spec_exit"][r]), (name, r, "speculative entry and exit", e, x)
        fast = shard.p1_spec_entries(lay, specs)
        if all(m["spec_true"]) and all(h for h, _, _ in specs):
            assert fast is not None, (name, specs)
        if fast is not None:
            assert fast == m["entry"], (name, "a chain that holds gives the true entries", fast, m["entry"])
        tables = [s.exit_table() for s in shards]
        for r in range(world):
            k = len(m["table"][r])
            if tables[r][:k] != m["table"][r]:
                e = next(i for i in range(k) if tables[r][i] != m["table"][r][i])
                raise AssertionError("%s: exit table of rank %d, entry %d: %d, the model's %d" % (name, r, e, tables[r][e], m["table"][r][e]))
        entries = shard.p1_entries(lay, tables)
        assert entries == m["entry"], (name, entries, m["entry"])
        # ---- tokens
        toks = []
        for r in range(world):
            e = entries[r] - lay[r]["g_lo"]
            n, p = shards[r].emit(e)
            assert n == m["count"][r], (name, r, "token count", n, m["count"][r])
            _same_tokens(_words(p, n), m["tokens"][r], "%s rank %d" % (name, r))
            if reemit:  # an emit somewhere else takes the exact way; so does coming back to the true entry
                other = e + 1 if r else 1
                shards[r].emit(other)
                if other < lay[r]["hi"]:
                    assert not shards[r].spec()[0], (name, r)
                n, p = shards[r].emit(e)
                assert n == m["count"][r], (name, r, "token count the exact way", n, m["count"][r])
                _same_tokens(_words(p, n), m["tokens"][r], "%s rank %d the exact way" % (name, r))
            toks.append((n, p))
        # ---- blocks
        skip, tail, owns, pieces = shard.p1_token_plan([n for n, _ in toks])
        assert (skip, tail, owns, pieces) == (m["skip"], m["tail"], m["owns"], m["pieces"])
        costs = []
        for r in range(world):
            tail_ptr = 0
            if len(pieces[r]) == 1:
                tail_ptr = toks[pieces[r][0][0]][1]
            elif pieces[r]:
                t = torch.empty(tail[r], dtype=torch.int32, device="cuda:0")
                off = 0
                for q, k in pieces[r]:
                    shard.ctypes_copy_d2d(t.data_ptr() + 4 * off, toks[q][1], 4 * k)
                    off += k
                keep.append(t)
                tail_ptr = t.data_ptr()
            cs = shards[r].blocks(skip[r], tail_ptr, tail[r], owns[r])
            assert len(cs) == m["nblocks"][r], (name, r, "blocks owned", len(cs), m["nblocks"][r])
            costs.append(cs)
        allc = [x for cs in costs for x in cs]
        owner = [r for r in range(world) for _ in costs[r]]
        assert owner == [b["owner"] for b in m["blocks"]], (name, owner)
        for k, (x, b) in enumerate(zip(allc, m["blocks"])):
            assert (x[4], x[5]) == (b["in_bytes"], b["q13"]), (name, "block %d of rank %d: in_bytes, q13" % (k, owner[k]), x[4:], b)
        if m["ref"] is None and compat:
            with pytest.raises(da.DeflateError) as ei:
                da.plan_blocks(allc, compat)
            assert ei.value.code == da.E_REF_PANIC
            return None
        plans, total_bits = da.plan_blocks(allc, compat)
        if m["ref"] is not None:
            assert [(p[0], p[1], p[2]) for p in plans] == [(b["btype"], b["bfinal"], b["bit_start"]) for b in m["blocks"]], (name, plans)
            assert (total_bits + 7) // 8 == len(m["ref"]), (name, total_bits, len(m["ref"]))
        # ---- pack
        ref_bits = _bits(m["ref"]) if m["ref"] is not None else None
        flagged = [k for k, b in enumerate(m["blocks"]) if b["q13"] and plans[k][0] == 0]
        out = np.zeros((total_bits + 7) // 8 + 16, dtype=np.uint8)
        b0 = 0
        for r in range(world):
            nb = len(costs[r])
            mine = plans[b0:b0 + nb]
            end_bit = plans[b0 + nb][2] if b0 + nb < len(plans) else total_bits
            mine_k = range(b0, b0 + nb)
            b0 += nb
            if not nb:
                continue
            first_bit = mine[0][2]
            want_bytes = (end_bit - first_bit // 32 * 32 + 7) // 8
            cap = want_bytes + 64
            dev = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
            fb, nbytes = shards[r].pack(mine, end_bit, dev.data_ptr(), cap)
            assert fb % 4 == 0 and fb == first_bit // 32 * 4 and nbytes == want_bytes, (name, r, fb, nbytes)
            host = dev.cpu().numpy()
            cleared = (nbytes + 8 + 3) // 4 * 4
            assert not host[nbytes:cleared].any() and (host[cleared:] == 0xA5).all(), (name, r, "bytes behind the rank's own")
            got = _bits(host[:nbytes])
            lo, hi = first_bit - 8 * fb, end_bit - 8 * fb
            assert not got[:lo].any() and not got[hi:].any(), (name, r, "a bit outside the rank's own bit range [%d, %d)" % (first_bit, end_bit),
                                                             np.flatnonzero(got[:lo])[:4], hi + np.flatnonzero(got[hi:])[:4])
            if ref_bits is not None and (compat or not any(k in flagged for k in mine_k)):
                want = ref_bits[first_bit:end_bit]
                if not np.array_equal(got[lo:hi], want):
                    i = int(np.argmax(got[lo:hi] != want))
                    raise AssertionError("%s: rank %d's bits differ from the oracle's at stream bit %d (its range is [%d, %d))" % (name, r, first_bit + i, first_bit, end_bit))
            out[fb:fb + nbytes] |= host[:nbytes]
        return out[:(total_bits + 7) // 8].tobytes()
    except da.DeflateError as e:
        if e.code == da.E_HIP:  # (a device error: nothing more is started on this GPU)
            pytest.exit("HIP error in %s: %s" % (name, e), returncode=3)
        raise
    finally:
        for s in shards:
            s.close()


def run_case(da, ctxs, name, reemit=False):
    c = sc.case(name)
    m = sc.model_of(c)
    got = drive(da, ctxs, c, 1, reemit)
    assert got == m["ref"], (name, "the stitched stream")
    if not m["hazards"]:
        assert zlib.decompress(got, -15) == c["data"]
    # the driver itself on the same cuts
    real = shard.encode_p1_virtual(da, ctxs[:m["world"]], c["data"], da.CompressionOptions(*c["opts"]), compat=1, layouts=m["lay"])
    assert real == m["ref"], (name, "shard.encode_p1_virtual")


@pytest.mark.parametrize("name", sc.names("seam") + sc.names("short"))
def test_seams_and_short_ranges_by_speculation_and_the_exact_way(da, ctxs, name):
    """with the steps worked out by k_emit and filed by k_adv, and with the tokens made a second time the exact way"""
    try:
        for where in (0, 1):
            for c in ctxs:
                c.config(da.Context.CFG_STEPS_IN_EMIT, where)
            run_case(da, ctxs, name, reemit=True)
    finally:
        for c in ctxs:
            c.config(da.Context.CFG_STEPS_IN_EMIT, 1)


@pytest.mark.parametrize("name", [n for f in ("count", "last", "halo", "stored", "levels") for n in sc.names(f)])
def test_counts_last_ranges_halos_stored_blocks_and_levels(da, ctxs, name):
    run_case(da, ctxs, name)


@pytest.mark.parametrize("name", sc.names("q13"))
def test_q13_block_cut_by_ranks(da, ctxs, name):
    c = sc.case(name)
    m = sc.model_of(c)
    if m["ref"] is None:  # the reference panics: so does the plan, asked for its bytes; the real bytes make a valid stream
        assert drive(da, ctxs, c, da.COMPAT_Q13) is None
        got = drive(da, ctxs, c, 0)
        assert zlib.decompress(got, -15) == c["data"]
        return
    run_case(da, ctxs, name)  # (with MI355_COMPAT_Q13: the reference's bytes)
    got = drive(da, ctxs, c, 0)
    assert zlib.decompress(got, -15) == c["data"], name
    k = next(i for i, b in enumerate(m["blocks"]) if b["q13"])
    lo, hi = m["blocks"][k]["bit_start"] // 8, (m["blocks"][k + 1]["bit_start"] + 7) // 8
    assert len(got) == len(m["ref"]) and got[:lo] == m["ref"][:lo] and got[hi:] == m["ref"][hi:] and got != m["ref"], name


@pytest.mark.parametrize("total,world", [(8192, 8), (20_000, 3), (100_000, 8), (262_143, 8)])
def test_small_inputs_over_several_ranks(da, ctxs, total, world):
    """less than 32 KiB per rank: shard.p1_layout cuts at multiples of 1024 (before: anywhere, and mi355_shard_begin refused)"""
    data = sc._text(total, 70 + world)
    lay = [shard.p1_layout(total, r, world) for r in range(world)]
    assert all(L["b"] - L["a"] < 32768 for L in lay[:-1]) and all(L["a"] % sc.SEG == 0 for L in lay)
    got = shard.encode_p1_virtual(da, ctxs[:world], data, da.Compression.Default, compat=1)
    assert got == ob.encode(data, opts=ob.make_opts(*sc.DEFAULT)) and zlib.decompress(got, -15) == data


def test_q13_block_needs_the_bytes_the_reference_reads(da, ctxs):
    """Under MI355_COMPAT_Q13 the flagged Stored block's bytes are read 32768 further on: its owner must hold them.  The block ends
    at 98328, so a rank 0 that holds 131096 bytes gives the reference's stream, and one that holds a byte less is refused by
    mi355_shard_pack -- not handed zeros for the bytes it does not have.  Asked for the real bytes, the shorter buffer will do."""
    base = sc.case("q13/seed1_66560")
    k = next(i for i, b in enumerate(sc.model_of(base)["blocks"]) if b["q13"])
    end = sc.model_of(base)["blocks"][k]["start"] + sc.model_of(base)["blocks"][k]["in_bytes"]
    assert end == 98328
    enough = dict(base, name="q13/seed1_66560_holds_%d" % (end + sc.WINDOW), g_hi=[end + sc.WINDOW, None])
    short = dict(base, name="q13/seed1_66560_holds_%d" % (end + sc.WINDOW - 1), g_hi=[end + sc.WINDOW - 1, None])
    for c in (enough, short):
        sc.check(c)
    assert drive(da, ctxs, enough, da.COMPAT_Q13) == sc.model_of(enough)["ref"]
    with pytest.raises(da.DeflateError) as ei:
        drive(da, ctxs, short, da.COMPAT_Q13)
    assert ei.value.code == da.E_ARG and "look-ahead" in str(ei.value), ei.value
    assert zlib.decompress(drive(da, ctxs, short, 0), -15) == base["data"]
    assert ctxs[0].encode(base["data"][:5000], da.Compression.Default) == ob.encode(base["data"][:5000], opts=ob.make_opts(*sc.DEFAULT))


def test_refusals_leave_the_context_usable(da, ctxs):
    data = sc.case("halo/look_ahead_257")["data"]
    n = len(data)
    ref = ob.encode(data, opts=ob.make_opts(*sc.DEFAULT))
    ctx, other = ctxs[0], ctxs[1]
    buf = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).to("cuda:0")

    def refused(code, f, *a):
        with pytest.raises(da.DeflateError) as ei:
            f(*a)
        assert ei.value.code == code, (ei.value.code, code)

    def begin(c, lo, hi=n):
        return da.Shard(c, buf.data_ptr(), n, lo, hi, 0, n, da.Compression.Default, 1)

    for lo in (1, 512, 1023, 1025):
        refused(da.E_ARG, begin, ctx, lo)
    assert ctx.encode(data, da.Compression.Default, compat=1) == ref
    s = begin(ctx, 0)
    try:
        refused(da.E_STATE, begin, ctx, 0)                                         # a second begin on a busy context
        refused(da.E_STATE, ctx.encode, data, da.Compression.Default)              # an encode on a busy context
        n_tok, _ = s.emit(0)
        assert n_tok == len(ob.lz77(data, *sc.DEFAULT)) and n_tok % sc.BLOCK
        refused(da.E_ARG, s.blocks, n_tok + 1, 0, 0, True)                          # skip > T
        refused(da.E_ARG, s.blocks, 0, 0, 0, False)                                # a non-owner with a partial block
        # the shard goes on as if nothing had been asked
        costs = s.blocks(0, 0, 0, True)
        plans, bits = da.plan_blocks(costs, 1)
        dev = torch.zeros(bits // 8 + 64, dtype=torch.uint8, device="cuda:0")
        fb, nbytes = s.pack(plans, bits, dev.data_ptr(), dev.numel())
        assert fb == 0 and bytes(dev[:nbytes].cpu().numpy()) == ref
    finally:
        s.close()
    s = begin(other, 1024)
    try:
        for e in (0, 1023):
            refused(da.E_ARG, s.emit, e)                                           # emit below parse_lo
        m = sc.model_of(dict(name="refusals", data=data, opts=sc.DEFAULT, cuts=[0, 1024]))
        n_tok, p = s.emit(m["entry"][1])
        assert n_tok == m["count"][1]
        _same_tokens(_words(p, n_tok), m["tokens"][1], "after the refused emits")
    finally:
        s.close()
    for c in (ctx, other):
        assert c.encode(data, da.Compression.Default, compat=1) == ref
