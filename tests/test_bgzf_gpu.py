"""The BGZF encode (mi355_bgzf_encode[_device]) on the GPU against the model of bgzf_cases.py: for every case the return value,
*out_len, the bytes and the member table, with 64 guard bytes of fill behind out_cap untouched -- at the bound, at the exact size and
one byte short of it; the size query; the host entry against the device entry; the round trip through mi355_inflate_members; the
interleaved case with the one-input path proved taken; the errors of the call.  All cases run on one context.  pytest -m gpu."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))

import bgzf_cases as bc

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
BATCH_BYTES_DEFAULT = 256 << 20
CASES = bc.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def da():
    import deflate_amd
    return deflate_amd


@pytest.fixture(scope="module")
def ctx(da):
    c = da.Context(0)
    yield c
    c.close()


_DEV = {}


def on_device(data):
    """the input as a device tensor, uploaded once (None for the empty input)"""
    if data not in _DEV:
        _DEV[data] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else None
        torch.cuda.synchronize()
    return _DEV[data]


def opts(da, case):
    return da.CompressionOptions(*bc.LEVELS[case.level][1])


def run_device(da, ctx, case, cap, room=None, compat=0):
    """the device entry into a buffer of `cap` bytes with GUARD bytes of FILL behind them: (rc, out_len, n_members, members, the
    buffer's first cap bytes); the guard is checked here"""
    t = on_device(case.data)
    out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert out.data_ptr() % 16 == 0
    if case.batch_bytes:
        ctx.config(da.Context.CFG_BATCH_BYTES, case.batch_bytes)
    try:
        rc, n, nm, members = ctx.encode_bgzf_device(t.data_ptr() if t is not None else 0, len(case.data), out.data_ptr(), cap, opts(da, case),
                                                    case.block, compat=compat, room=room, check=False)
    finally:
        if case.batch_bytes:
            ctx.config(da.Context.CFG_BATCH_BYTES, BATCH_BYTES_DEFAULT)
    raw = out.cpu().numpy().tobytes()
    assert raw[cap:] == bytes([FILL]) * GUARD, "the device entry wrote behind out_cap"
    return rc, n, nm, members, raw[:cap]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_entry_gives_the_models_file_and_table(da, ctx, case):
    file, members = bc.model(case.data, case.level, case.block)
    bound = da.bgzf_bound(len(case.data), case.block)
    rc, n, nm, got, raw = run_device(da, ctx, case, bound)
    print("%s: rc %d, %d bytes in %d members (model %d in %d), bound %d" % (case.name, rc, n, nm, len(file), len(members), bound))
    assert rc == da.OK
    assert n == len(file)
    assert raw[:n] == file
    assert nm == len(members) and got == members


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_exact_size_is_enough_and_one_byte_less_is_not(da, ctx, case):
    file, members = bc.model(case.data, case.level, case.block)
    rc, n, nm, got, raw = run_device(da, ctx, case, len(file))
    assert (rc, n, nm) == (da.OK, len(file), len(members))
    assert raw == file and got == members
    rc, n, nm, _got, _raw = run_device(da, ctx, case, len(file) - 1)
    assert (rc, n, nm) == (da.E_OUT_TOO_SMALL, len(file), len(members))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_size_query_and_host_entry(da, ctx, case):
    file, members = bc.model(case.data, case.level, case.block)
    if case.batch_bytes:
        ctx.config(da.Context.CFG_BATCH_BYTES, case.batch_bytes)
    try:
        t = on_device(case.data)
        rc, n, nm, got = ctx.encode_bgzf_device(t.data_ptr() if t is not None else 0, len(case.data), 0, 0, opts(da, case), case.block,
                                                room=0, check=False)
        assert (rc, n, nm, got) == (da.E_OUT_TOO_SMALL, len(file), len(members), [])
        rc, n, nm, got, buf = ctx.encode_bgzf_raw(case.data, opts(da, case), case.block, out_cap=0, room=3)
        assert (rc, n, nm, got) == (da.E_OUT_TOO_SMALL, len(file), len(members), members[:3])  # (the table is cut without an error)
        data, got = ctx.encode_bgzf(case.data, opts(da, case), case.block)
        assert data == file and got == members
    finally:
        if case.batch_bytes:
            ctx.config(da.Context.CFG_BATCH_BYTES, BATCH_BYTES_DEFAULT)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_round_trip_through_inflate_members(da, ctx, case):
    file, members = ctx.encode_bgzf(case.data, opts(da, case), case.block)
    data, walked = ctx.inflate_members(file)
    assert data == case.data
    assert walked == members
    assert all(m["flags"] == da.MEMBER_HINTED and m["status"] == "OK" for m in walked)
    assert da.bgzf_gzi(members) == bc.gzi(bc.model(case.data, case.level, case.block)[1])


def test_the_interleaved_case_takes_the_one_input_path_between_batched_slices(da, ctx):
    (case,) = bc.interleaved()
    file, members = bc.model(case.data, case.level, case.block)
    rc, n, _nm, got, raw = run_device(da, ctx, case, da.bgzf_bound(len(case.data), case.block))
    assert rc == da.OK and raw[:n] == file and got == members
    bi = ctx.batch_info()
    print("interleaved:", bi)
    assert bi["n_items"] == 8 and bi["n_single"] > 0 and bi["n_batched"] > 0 and bi["n_single"] + bi["n_batched"] == 8
    assert bi["n_q1_single"] > 0 and bi["n_spec_single"] > 0  # (noise fires Q1, zeros fail the speculative parse)
    info = ctx.info()
    assert info["in_len"] == len(case.data) and info["out_len"] == len(file) - 28  # (as after the packed batch: the members' bytes)
    assert ctx.blocks() == []


def test_the_launch_sets_are_cut_and_do_not_show(da, ctx):
    (case,) = bc.sets()
    file, _members = bc.model(case.data, case.level, case.block)
    rc, n, _nm, _got, raw = run_device(da, ctx, case, len(file))
    assert rc == da.OK and raw == file
    # the packed batch's rule: consecutive items while their bytes, header included, stay within the setting -- 16 slices of
    # 65280 + 18 bytes to the MiB, so the 49 slices of 3 MiB make four sets, the last of one slice
    sets, room = 0, 0
    for s in bc.slices(case.data, case.block):
        if sets == 0 or room + len(s) + len(bc.H) > case.batch_bytes:
            sets, room = sets + 1, 0
        room += len(s) + len(bc.H)
    assert ctx.batch_info()["sub_batches"] == sets == 4


def test_stage_clocks(da, ctx):
    (case,) = bc.sets()
    assert set(ctx.bgzf_stages()) == {"packed_encode_ms", "place_ms", "gather_ms"}
    ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
    try:
        run_device(da, ctx, case, da.bgzf_bound(len(case.data), case.block))
        ms = ctx.bgzf_stages()
        assert all(v > 0 for v in ms.values()), ms
    finally:
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
    run_device(da, ctx, case, da.bgzf_bound(len(case.data), case.block))
    assert all(v == 0 for v in ctx.bgzf_stages().values())


def test_errors_of_the_call(da, ctx):
    L = da.load()
    (case,) = [c for c in CASES if c.name == "edge-65281"]
    file, _members = bc.model(case.data, case.level, case.block)
    t = on_device(case.data)
    out = torch.full((len(file) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, nm = C.c_size_t(0), C.c_size_t(0)

    def call(o, block=0, d_out=None, flush=0):
        o = o.to_c(0, 0, flush)  # (the wrapper is taken as 2 whatever it holds)
        return L.mi355_bgzf_encode_device(ctx._h, C.c_void_p(t.data_ptr()), len(case.data), C.byref(o), block,
                                          C.c_void_p(out.data_ptr() if d_out is None else d_out), len(file), C.byref(n), None, 0, C.byref(nm), None)

    assert call(da.CompressionOptions(128, 2, 1)) == da.E_UNSUPPORTED  # lazy_if_less_than < 3 with Lazy
    assert call(da.CompressionOptions.default(), flush=1) == da.E_ARG  # FINISH only
    assert call(da.CompressionOptions.default(), block=65281) == da.E_ARG
    assert call(da.CompressionOptions.default(), d_out=out.data_ptr() + 8) == da.E_ARG
    assert out.cpu().numpy().tobytes() == bytes([FILL]) * (len(file) + GUARD)  # (a refused call writes nothing)
    # a context that holds a sharded encode refuses, and works again afterwards (a context of its own: the shard is its state)
    own = da.Context(0)
    d = torch.frombuffer(bytearray(case.data + bytes(64)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    sh = C.c_void_p()
    o = da.CompressionOptions.default().to_c()
    assert L.mi355_shard_begin(own._h, d.data_ptr(), len(case.data), 0, len(case.data), 0, len(case.data), C.byref(o), None, C.byref(sh)) == da.OK
    try:
        assert L.mi355_bgzf_encode_device(own._h, C.c_void_p(t.data_ptr()), len(case.data), C.byref(o), 0, C.c_void_p(out.data_ptr()), len(file),
                                          C.byref(n), None, 0, C.byref(nm), None) == da.E_STATE
        assert L.mi355_bgzf_encode(own._h, case.data, len(case.data), C.byref(o), 0, None, 0, C.byref(n), None, 0, None) == da.E_STATE
    finally:
        L.mi355_shard_end(sh)
    assert own.encode_bgzf(case.data)[0] == file
    own.close()
    assert out.cpu().numpy().tobytes() == bytes([FILL]) * (len(file) + GUARD)  # (a refused call writes nothing)
    assert call(da.CompressionOptions.default()) == da.OK and n.value == len(file) and nm.value == 3
    assert out.cpu().numpy().tobytes() == file + bytes([FILL]) * GUARD


def test_compat_q13_changes_nothing_for_slices_this_short(da, ctx):
    """MI355_E_REF_PANIC needs a stored block in a window behind the first (A.4 Q13), which no slice of 65280 bytes or fewer has: under
    the compat bit the longest members there are come out as the model's"""
    (case,) = [c for c in bc.noise() if c.level == "default"]
    file, members = bc.model(case.data, case.level, case.block)
    rc, n, _nm, got, raw = run_device(da, ctx, case, len(file), compat=da.COMPAT_Q13)
    assert rc == da.OK and raw == file and got == members
