"""The verify entry points on the device (include/mi355_deflate.h mi355_deflate_verify*): the encoder's own streams verify with
and without the block table and through the host entry; the reference's Q13 stream does not; and every mutated, hand-assembled
and edited case of verify_cases.py gets from k_verify the report the host build of the same decisions gives.
Needs a real MI355X: pytest -m gpu."""
import os
import sys

import pytest
import torch  # noqa: F401  -- before the library (see test_gpu_parity.py)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import inflcheck_binding as ib
import verify_cases as vc

pytestmark = pytest.mark.gpu

LV = {"fast": (1, 0, 0), "default": (128, 32, 1), "best": (1768, 128, 1), "rle": (0, 0, 1), "huffman_only": (0, 0, 0)}
KEY = ("status", "entry", "bit", "in_pos")


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


def verify_dev(ctx, stream, data, wrapper, blocks=None):
    s, d = dev(stream), dev(data)
    return ctx.verify_device(s.data_ptr(), len(stream), d.data_ptr(), len(data), wrapper, blocks)


def encoder_inputs():
    import header_cases
    with open(os.path.join(vc.FIX, "short.bin"), "rb") as f:
        short = f.read()
    return [("pg11", vc.pg11()), ("short.bin", short), ("empty", b""), ("one_byte", b"Q"), ("noise_200k", vc.noise(200000, 3)),
            ("zeros_70000", bytes(70000)), ("header_case", bytes(header_cases.case(header_cases.names()[0])[1]))]


@pytest.mark.parametrize("level", list(LV))
def test_encoder_streams_verify(da, ctx, level):
    for name, data in encoder_inputs():
        for wrapper in (0, 1, 2):
            stream = ctx.encode(data, da.CompressionOptions(*LV[level]), wrapper=wrapper)
            blocks = ctx.blocks()
            info = ctx.info()
            for how, (rc, rep) in (("device, table", verify_dev(ctx, stream, data, wrapper, blocks or None)),
                                   ("device, no table", verify_dev(ctx, stream, data, wrapper)),
                                   ("host, table", ctx.verify(stream, data, wrapper, blocks or None))):
                assert (rc, rep["status"]) == (da.OK, "OK"), (name, level, wrapper, how, rep)
                assert (rep["n_fixed"], rep["n_dynamic"]) == (info["n_fixed"], info["n_dynamic"]), (name, level, wrapper, how, rep)
                assert rep["n_blocks"] == rep["n_stored"] + rep["n_fixed"] + rep["n_dynamic"]
            assert ctx.blocks() == blocks and ctx.info()["out_len"] == info["out_len"]  # the encode's records are undisturbed


def test_q13_the_references_stream_does_not_verify(da, ctx):
    from test_stages_vs_oracle import q13_case
    d = next(x for x in (q13_case(seed) for seed in (1, 2, 3)) if x is not None)
    good = ctx.encode(d, da.Compression.Default, compat=0)
    assert ctx.verify(good, d, 0, ctx.blocks())[0] == da.OK
    assert verify_dev(ctx, good, d, 0)[0] == da.OK
    bad = ctx.encode(d, da.Compression.Default, compat=da.COMPAT_Q13)
    assert ctx.info()["q13_hits"] >= 1
    blocks = ctx.blocks()
    rc, rep = ctx.verify(bad, d, 0, blocks)
    assert rc == da.E_VERIFY and rep["status"] != "OK", rep
    assert rep == dict(ib.verify(bad, d, 0, [(b["bit_start"], b["in_bytes"]) for b in blocks])[1], ms=rep["ms"])
    rc, rep = verify_dev(ctx, bad, d, 0)
    assert rc == da.E_VERIFY and key(rep) == key(ib.verify(bad, d, 0)[1]), rep
    with pytest.raises(da.DeflateError) as e:
        ctx.encode(d, da.Compression.Default, compat=da.COMPAT_Q13, verify=True)
    assert e.value.code == da.E_VERIFY


@pytest.mark.parametrize("wrapper", [0, 1, 2])
def test_corpora_through_the_batch_entry_match_the_host_build(da, ctx, wrapper):
    """one launch per wrapper: the mutated, hand-assembled and edited cases, and the valid streams, as the items of one batch"""
    cases = [c[:4] for c in vc.mutations() + vc.hand() + vc.edits() + vc.streams() if c[3] == wrapper]
    assert len(cases) > (600 if wrapper < 2 else 20)
    blob_s = dev(b"".join(c[1] for c in cases))
    inputs, in_at, blob = {}, 0, []
    for c in cases:  # (many cases share an input: one copy each)
        if c[2] not in inputs:
            inputs[c[2]] = in_at
            blob.append(c[2])
            in_at += len(c[2])
    blob_i = dev(b"".join(blob))
    items, at = [], 0
    for c in cases:
        items.append((blob_s.data_ptr() + at, len(c[1]), blob_i.data_ptr() + inputs[c[2]], len(c[2])))
        at += len(c[1])
    rc, statuses, reps = ctx.verify_batch_device(items, wrapper)
    n_bad = 0
    for c, st, rep in zip(cases, statuses, reps):
        want_rc, want = ib.verify(c[1], c[2], wrapper)
        assert key(rep) == key(want) and st == want_rc, (c[0], rep, want)
        if want_rc == da.OK:
            assert {k: rep[k] for k in rep if k != "ms"} == want, (c[0], rep, want)
        n_bad += want_rc != da.OK
    assert rc == (da.E_VERIFY if n_bad else da.OK) and (n_bad > 0 or wrapper == 2)
    rc2, statuses2, reps2 = ctx.verify_batch_device(items, wrapper)  # a function of the arguments alone
    assert (rc2, statuses2, [key(r) for r in reps2]) == (rc, statuses, [key(r) for r in reps])


def test_with_a_table_the_failing_entry_is_named(da, ctx):
    data = vc.pg11()
    stream = ctx.encode(data, da.CompressionOptions(*LV["huffman_only"]))
    blocks = ctx.blocks()
    table = [(b["bit_start"], b["in_bytes"]) for b in blocks]
    assert len(table) >= 6
    assert verify_dev(ctx, stream, data, 0, blocks)[0] == da.OK

    def both(s, t):
        rc, rep = verify_dev(ctx, s, data, 0, t)
        want_rc, want = ib.verify(s, data, 0, t)
        assert rc == want_rc == da.E_VERIFY and key(rep) == key(want), (rep, want)
        assert key(ctx.verify(s, data, 0, t)[1]) == key(want)
        return rep

    off = list(table)
    off[3] = (off[3][0] + 1, off[3][1])
    rep = both(stream, off)
    assert rep["status"] == "TABLE" and rep["entry"] in (2, 3)

    def flip(s, entry):
        m = bytearray(s)
        bit = (table[entry][0] + table[entry + 1][0]) // 2 if entry + 1 < len(table) else table[entry][0] + 4000
        m[bit >> 3] ^= 1 << (bit & 7)
        return bytes(m)

    assert both(flip(stream, 4), table)["entry"] == 4
    assert both(flip(flip(stream, 5), 2), table)["entry"] == 2


def test_batch_of_encoder_streams(da, ctx):
    text = vc.pg11()
    datas = [text[4096 * k: 4096 * (k + 1)] for k in range(40)] + [vc.noise(4096, k) for k in range(24)] + [(text * 19)[: 3 << 20]]
    ins = [dev(d) for d in datas]
    # unpacked
    outs, lens, sts = ctx.encode_batch_device(ins, options=da.Compression.Default, wrapper=1)
    assert all(s == da.OK for s in sts)
    binfo = ctx.batch_info()
    items = [(o.data_ptr(), n, i.data_ptr(), len(d)) for o, n, i, d in zip(outs, lens, ins, datas)]
    rc, statuses, reps = ctx.verify_batch_device(items, 1)
    assert rc == da.OK and all(s == da.OK for s in statuses) and all(r["status"] == "OK" for r in reps)
    assert ctx.batch_info() == binfo
    outs[7][lens[7] // 2] ^= 0x10   # item 7: its stream corrupted
    ins[20][100] ^= 0x01            # item 20: its input changed
    torch.cuda.synchronize()
    items[33] = items[33] + (da.E_OUT_TOO_SMALL,)  # item 33: not OK on entry -- skipped, left alone
    rc, statuses, reps = ctx.verify_batch_device(items, 1)
    assert rc == da.E_VERIFY
    assert [k for k, s in enumerate(statuses) if s != da.OK] == [7, 20, 33]
    assert statuses[7] == statuses[20] == da.E_VERIFY and statuses[33] == da.E_OUT_TOO_SMALL
    assert reps[20]["status"] in ("MISMATCH", "CHECKSUM") and reps[33]["status"] == "OK" and reps[33]["n_blocks"] == 0
    assert ctx.batch_info() == binfo
    ins[20][100] ^= 0x01
    torch.cuda.synchronize()
    # packed, gzip: the entries' places in the arena
    res = ctx.encode_batch_packed_device(ins, options=da.Compression.Default, wrapper=2, align=8)
    base = res.arena.data_ptr()
    items = [(base + off, n, i.data_ptr(), len(d)) for (off, n), i, d in zip(res.entries, ins, datas)]
    rc, statuses, reps = ctx.verify_batch_device(items, 2)
    assert rc == da.OK and all(s == da.OK for s in statuses)
    res.arena[res.entries[64][0] + res.entries[64][1] // 3] ^= 0x40  # the 3 MiB item
    torch.cuda.synchronize()
    rc, statuses, reps = ctx.verify_batch_device(items, 2)
    assert rc == da.E_VERIFY and [k for k, s in enumerate(statuses) if s != da.OK] == [64]


def test_encode_with_verify_returns_the_same_bytes(da, ctx):
    data = vc.pg11()
    for wrapper in (0, 1, 2):
        assert ctx.encode(data, da.Compression.Default, wrapper=wrapper, verify=True) == ctx.encode(data, da.Compression.Default, wrapper=wrapper)
    hdr = vc.GZ_HEADERS["all"]
    assert ctx.encode_gzip(data, da.Compression.Best, header=hdr, verify=True) == ctx.encode_gzip(data, da.Compression.Best, header=hdr)
    assert ctx.encode(b"", verify=True) == ctx.encode(b"")
    ok, rep = da.verify_bytes(ctx.encode(data, wrapper=1), data, 1, ctx=ctx)
    assert ok and rep["status"] == "OK"
    ok, rep = da.verify_bytes(ctx.encode(data, wrapper=1), data[:-1] + b"!", 1, ctx=ctx)
    assert not ok and (rep["status"], rep["in_pos"]) == ("MISMATCH", len(data) - 1)


def test_arguments(da, ctx):
    data = vc.pg11()
    stream = ctx.encode(data, da.CompressionOptions(*LV["huffman_only"]))
    table = [(b["bit_start"], b["in_bytes"]) for b in ctx.blocks()]
    for bad_wrapper, bad_table in ((3, table), (-1, table), (0, [table[1], table[0]] + table[2:]), (0, table[:-1]),
                                   (0, table[:-1] + [(table[-1][0], table[-1][1] + 1)])):
        with pytest.raises(da.DeflateError) as e:
            ctx.verify(stream, data, bad_wrapper, bad_table)
        assert e.value.code == da.E_ARG
        with pytest.raises(da.DeflateError) as e:
            verify_dev(ctx, stream, data, bad_wrapper, bad_table)
        assert e.value.code == da.E_ARG
    with pytest.raises(da.DeflateError) as e:
        ctx.verify_batch_device([(0, 0, 0, 0)], 3)
    assert e.value.code == da.E_ARG
