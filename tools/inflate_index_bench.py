"""tools/inflate_index_bench.py -- what the parallel inflate of ONE large stream costs when nobody kept its block table, against the
tabled inflate that has the encoder's table and against the one-wave inflate.

One MI355X, device-resident data, best of --reps (default 5), the runs of a group alternating in one session, on the 100 MB text of
bench.py as two streams: (i) encoded by this library at Default, (ii) deflated by Python's zlib at level 6.  Per stream:
  parallel  mi355_inflate_parallel_device, raw and zlib
  stages    the same raw call with MI355_CFG_STAGE_CLOCKS on, a context of its own: find (k_index_find), walk (k_index_walk), the
            host's link, and the tabled pass's decode / windows / resolve
  sweep     the raw call at MI355_CFG_INFLATE_INDEX_SPAN_BYTES = 16, 32, 64 and 128 KiB, the four alternating
  tabled    stream (i) only: mi355_inflate_tabled_device of the baseline library with the encoder's own table
  one_wave  mi355_inflate_device, ONE wave, run once (--one-wave 0 leaves it out)
The baseline library is the file MI355_BASELINE_LIB names (a build of the parent commit) and this tree's own library when the
variable is not set; the result says which it was.  Every timed call returns after its stream has drained; every output is compared
with the input once, outside the timing.
Writes profiles/inflate_index_bench.json (--out) and prints the same JSON line.  --size N: bytes of the text (default 100 000 000)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

SWEEP = (16 << 10, 32 << 10, 64 << 10, 128 << 10)


def baseline_library():
    """(the library the tabled inflate is timed on, a context of it, what it is)"""
    path = os.environ.get("MI355_BASELINE_LIB", "")
    if not path:
        return da.load(), None, "this tree's library"
    B = C.CDLL(path)
    B.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    B.mi355_inflate_tabled_device.argtypes = da.load().mi355_inflate_tabled_device.argtypes
    h = C.c_void_p()
    rc = B.mi355_deflate_ctx_create(0, C.byref(h))
    assert rc == 0, rc
    return B, h, "MI355_BASELINE_LIB"


def alternate(fns, reps):
    """every function once to warm, then reps rounds in turn: {name: (best ms, spread ms)}"""
    for k, fn in fns.items():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (min(v), max(v) - min(v)) for k, v in times.items()}


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--one-wave", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_index_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    B, bh, which = baseline_library()
    bh = bh or ctx._h
    res = {"metric": "parallel inflate of one stream without its table (best of %d, alternating runs, device-resident)" % a.reps,
           "baseline": which, "device": torch.cuda.get_device_name(0)}
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    d_in = dev(data)
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    got, irep = C.c_size_t(0), da.InflateReport()
    # (i): this library at Default, raw and zlib, with the encoder's table for the baseline
    cap = L.mi355_deflate_bound(len(data)) + 64
    own = {}
    for wrapper in (0, 1):
        d_s = torch.empty(cap, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(d_in.data_ptr(), len(data), d_s.data_ptr(), cap, da.Compression.Default, wrapper=wrapper)
        own[wrapper] = (d_s, n) + ctx._block_table(ctx.blocks())
    # (ii): Python's zlib at level 6
    z = zlib.compress(data, 6)
    theirs = {0: (dev(z[2:-4]), len(z) - 6), 1: (dev(z), len(z))}

    def parallel(s, wrapper, h=None):
        rc = L.mi355_inflate_parallel_device(h or ctx._h, C.c_void_p(s[0].data_ptr()), s[1], wrapper, C.c_void_p(d_out.data_ptr()), len(data),
                                             C.byref(got), C.byref(irep), None)
        assert rc == 0 and got.value == len(data), (rc, irep.as_dict())

    def tabled(wrapper):
        d_s, n, arr, nb = own[wrapper]
        rc = B.mi355_inflate_tabled_device(bh, C.c_void_p(d_s.data_ptr()), n, wrapper, arr, nb, C.c_void_p(d_out.data_ptr()), len(data),
                                           C.byref(got), C.byref(irep), None)
        assert rc == 0 and got.value == len(data), (rc, irep.as_dict())

    def check(fn):  # outside the timing: the bytes
        d_out.zero_()
        fn()
        assert torch.equal(d_out, d_in)

    clk = da.Context(0)
    clk.config(da.Context.CFG_STAGE_CLOCKS, 1)
    for name, streams in (("own_default", own), ("zlib_6", theirs)):
        fns = {"parallel_raw": lambda: parallel(streams[0], 0), "parallel_zlib": lambda: parallel(streams[1], 1)}
        if streams is own:
            fns["tabled_raw"] = lambda: tabled(0)
            fns["tabled_zlib"] = lambda: tabled(1)
        t = alternate(fns, a.reps)
        for fn in fns.values():
            check(fn)
        r = {"bytes": len(data), "stream_bytes": streams[0][1], "entries": len(ctx.inflate_index_device(streams[0][0].data_ptr(), streams[0][1], 0)),
             "span_bytes": SPAN_DEFAULT}
        for k, (best, spread) in t.items():
            r[k + "_ms"], r[k + "_spread_ms"] = round(best, 3), round(spread, 3)
        r["parallel_gbps"] = round(len(data) / t["parallel_raw"][0] / 1e6, 2)
        if streams is own:
            r["entries_of_the_encoder"] = own[0][3]
            r["parallel_over_tabled"] = round(t["parallel_raw"][0] / t["tabled_raw"][0], 3)
        # per launch: a context with the stage clocks on
        rows = []
        for _ in range(a.reps + 1):
            parallel(streams[0], 0, clk._h)
            x, y = clk.inflate_index_stages(), clk.inflate_tabled_stages()
            rows.append([x["find_ms"], x["walk_ms"], x["link_ms"], y["decode_ms"], y["windows_ms"], y["resolve_ms"]])
        r["stages"] = dict(zip(("find_ms", "walk_ms", "link_ms", "decode_ms", "windows_ms", "resolve_ms"),
                               [round(min(row[k] for row in rows[1:]), 3) for k in range(6)]))
        # the span size
        def at(S):
            def run():
                ctx.config(da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, S)
                parallel(streams[0], 0)
            return run
        sweep = alternate({S: at(S) for S in SWEEP}, a.reps)
        for S in SWEEP:
            check(at(S))
        ctx.config(da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, SPAN_DEFAULT)
        r["sweep"] = {str(S): {"ms": round(sweep[S][0], 3), "spread_ms": round(sweep[S][1], 3)} for S in SWEEP}
        r["sweep_best_span_bytes"] = min(SWEEP, key=lambda S: sweep[S][0])
        if a.one_wave:
            d_out.zero_()
            t0 = time.perf_counter()
            rc = L.mi355_inflate_device(ctx._h, C.c_void_p(streams[0][0].data_ptr()), streams[0][1], 0, C.c_void_p(d_out.data_ptr()), len(data),
                                        C.byref(got), C.byref(irep), None)
            one = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and got.value == len(data) and torch.equal(d_out, d_in), (rc, irep.as_dict())
            r["one_wave_ms"] = round(one, 1)
            r["one_wave_over_parallel"] = round(one / t["parallel_raw"][0], 1)
        res[name] = r
    clk.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


SPAN_DEFAULT = 16 << 10  # the default of MI355_CFG_INFLATE_INDEX_SPAN_BYTES

if __name__ == "__main__":
    main()
