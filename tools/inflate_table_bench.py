"""tools/inflate_table_bench.py -- what the tabled inflate of ONE large stream costs, against the encode that made the stream and
the tabled verify of it.

One MI355X, device-resident data, best of --reps (default 5), the runs of the group alternating in one session, on the 100 MB text
of bench.py encoded at Default by this library:
  tabled    mi355_inflate_tabled_device with the encode's block table, raw and zlib (the difference is the checksum half)
  stages    the same raw and zlib calls with MI355_CFG_STAGE_CLOCKS on, a context of its own: HIP-event time per launch kind --
            decode (k_inflate_tab), window chain (k_inflate_tab_window), resolve (k_inflate_tab_resolve), checksums
  encode    mi355_deflate_encode_device of the baseline library on the same input
  verify    mi355_deflate_verify_device of the baseline library with the same table
  one_wave  mi355_inflate_device of the same stream, ONE wave, run once (--one-wave 0 leaves it out)
The baseline library is the file MI355_BASELINE_LIB names (a build of the parent commit: `make -C deflate-rs_amd` in a checkout of
it) and this tree's own library when the variable is not set -- encode and verify are the same text either way, and the result says
which it was.  Every timed call returns after its stream has drained; every inflate's output is compared with the input once,
outside the timing.
Writes profiles/inflate_table_bench.json (--out) and prints the same JSON line.  --size N: bytes of the text (default 100 000 000)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402


def baseline_library():
    """(the library encode and verify are timed on, a context of it, what it is)"""
    path = os.environ.get("MI355_BASELINE_LIB", "")
    if not path:
        return da.load(), None, "this tree's library"
    B = C.CDLL(path)
    B.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    B.mi355_deflate_ctx_destroy.argtypes = [C.c_void_p]
    B.mi355_deflate_ctx_destroy.restype = None
    B.mi355_deflate_encode_device.argtypes = da.load().mi355_deflate_encode_device.argtypes
    B.mi355_deflate_verify_device.argtypes = da.load().mi355_deflate_verify_device.argtypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--one-wave", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_table_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    B, bh, which = baseline_library()
    bh = bh or ctx._h
    res = {"metric": "tabled inflate of one stream against its encode and its tabled verify (best of %d, alternating runs, "
                     "device-resident)" % a.reps, "baseline": which, "device": torch.cuda.get_device_name(0)}
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = L.mi355_deflate_bound(len(data)) + 64
    streams = {}
    for wrapper in (0, 1):
        d_s = torch.empty(cap, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(d_in.data_ptr(), len(data), d_s.data_ptr(), cap, da.Compression.Default, wrapper=wrapper)
        streams[wrapper] = (d_s, n) + ctx._block_table(ctx.blocks())
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    base_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    opts = da.CompressionOptions.from_(da.Compression.Default).to_c(0, 0, 0)
    n_out, got = C.c_size_t(0), C.c_size_t(0)
    vrep, irep = da.VerifyReport(), da.InflateReport()

    def enc():
        rc = B.mi355_deflate_encode_device(bh, C.c_void_p(d_in.data_ptr()), len(data), C.byref(opts), C.c_void_p(base_out.data_ptr()),
                                           base_out.numel(), C.byref(n_out), None)
        assert rc == 0, rc

    def ver():
        d_s, n, arr, nb = streams[0]
        rc = B.mi355_deflate_verify_device(bh, C.c_void_p(d_s.data_ptr()), n, C.c_void_p(d_in.data_ptr()), len(data), 0, arr, nb,
                                           C.byref(vrep), None)
        assert rc == 0, (rc, vrep.as_dict())

    def inflate(wrapper, h=None):
        d_s, n, arr, nb = streams[wrapper]
        rc = L.mi355_inflate_tabled_device(h or ctx._h, C.c_void_p(d_s.data_ptr()), n, wrapper, arr, nb, C.c_void_p(d_out.data_ptr()),
                                           len(data), C.byref(got), C.byref(irep), None)
        assert rc == 0 and got.value == len(data), (rc, irep.as_dict())

    t = alternate({"encode": enc, "verify": ver, "inflate_raw": lambda: inflate(0), "inflate_zlib": lambda: inflate(1)}, a.reps)
    assert n_out.value == streams[0][1]
    for wrapper in (0, 1):  # outside the timing: the bytes
        d_out.zero_()
        inflate(wrapper)
        assert torch.equal(d_out, d_in), wrapper
    r = {"bytes": len(data), "stream_bytes": streams[0][1], "entries": streams[0][3], "deflate_blocks": irep.n_blocks}
    for k, (best, spread) in t.items():
        r[k + "_ms"], r[k + "_spread_ms"] = round(best, 3), round(spread, 3)
    r["inflate_over_verify"] = round(t["inflate_raw"][0] / t["verify"][0], 3)
    r["inflate_over_encode"] = round(t["inflate_raw"][0] / t["encode"][0], 3)
    r["inflate_gbps"] = round(len(data) / t["inflate_raw"][0] / 1e6, 2)
    res["text"] = r

    # ---- per launch kind: a context with the stage clocks on ----
    clk = da.Context(0)
    clk.config(da.Context.CFG_STAGE_CLOCKS, 1)
    ms = (C.c_float * 4)()
    best = {}
    for wrapper in (0, 1):
        rows = []
        for _ in range(a.reps + 1):
            inflate(wrapper, clk._h)
            assert L.mi355_inflate_tabled_last_stages(clk._h, ms) == 0
            rows.append(list(ms))
        best[wrapper] = [round(min(row[k] for row in rows[1:]), 3) for k in range(4)]
    res["stages"] = {"raw": dict(zip(("decode_ms", "windows_ms", "resolve_ms", "checksums_ms"), best[0])),
                     "zlib": dict(zip(("decode_ms", "windows_ms", "resolve_ms", "checksums_ms"), best[1]))}
    clk.close()

    # ---- the same stream through one wave, once ----
    if a.one_wave:
        d_s, n, _arr, _nb = streams[0]
        d_out.zero_()
        t0 = time.perf_counter()
        rc = L.mi355_inflate_device(ctx._h, C.c_void_p(d_s.data_ptr()), n, 0, C.c_void_p(d_out.data_ptr()), len(data), C.byref(got),
                                    C.byref(irep), None)
        one = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and got.value == len(data) and torch.equal(d_out, d_in), (rc, irep.as_dict())
        res["one_wave"] = {"ms": round(one, 1), "over_tabled": round(one / t["inflate_raw"][0], 1)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
