"""tools/inflate_bench.py -- what the inflate entry points cost, against the verify of the same streams and the encode that made them.

One MI355X, device-resident data, best of --reps (default 5), the runs of a group alternating in one session:
  batches  mi355_inflate_batch_device on 256 x 64 KiB and 1024 x 4 KiB of text, encoded at Default by this library, against
           mi355_deflate_verify_batch_device of the BASELINE library on the same items -- the same serial chain without the
           stores -- and against the baseline's mi355_deflate_encode_batch_device of them
  single   mi355_inflate_device of one stream, pg11.txt and 1 MiB of text, beside the tableless verify of it: ns per token
The baseline library is the file MI355_BASELINE_LIB names (a build of the parent commit: `make -C deflate-rs_amd` in a
checkout of it) and this tree's own library when the variable is not set; the result says which it was.  Every timed call
returns after its stream has drained, and every inflate's output is compared with the input once, outside the timing.
Writes profiles/inflate_bench.json (--out) and prints the same JSON line."""
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
    """(the library verify and encode are timed on, a context of it, what it is)"""
    path = os.environ.get("MI355_BASELINE_LIB", "")
    if not path:
        return da.load(), None, "this tree's library"
    B = C.CDLL(path)
    B.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    B.mi355_deflate_ctx_destroy.argtypes = [C.c_void_p]
    B.mi355_deflate_ctx_destroy.restype = None
    B.mi355_deflate_encode_batch_device.argtypes = da.load().mi355_deflate_encode_batch_device.argtypes
    B.mi355_deflate_verify_batch_device.argtypes = da.load().mi355_deflate_verify_batch_device.argtypes
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


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    B, bh, which = baseline_library()
    bh = bh or ctx._h
    opts = da.CompressionOptions.from_(da.Compression.Default).to_c(0, 0, 0)
    res = {"metric": "inflate against the baseline's verify and encode of the same items (best of %d, alternating runs, device-resident)" % a.reps,
           "baseline": which, "device": torch.cuda.get_device_name(0)}

    # ---- batches ----
    res["batches"] = {}
    for name, datas in (("256x64KiB", [datagen.text_like(64 << 10, 1000 + k) for k in range(256)]),
                        ("1024x4KiB", [datagen.text_like(4 << 10, 5000 + k) for k in range(1024)])):
        k = len(datas)
        ins = [dev(d) for d in datas]
        outs = [torch.empty(L.mi355_deflate_bound_ex(len(d), 0, 0, 0), dtype=torch.uint8, device="cuda") for d in datas]
        back = [torch.zeros(len(d), dtype=torch.uint8, device="cuda") for d in datas]
        e_items, v_items, i_items = (da.BatchItem * k)(), (da.BatchItem * k)(), (da.BatchItem * k)()
        for i, d in enumerate(datas):
            e_items[i].in_, e_items[i].in_len = C.c_void_p(ins[i].data_ptr()), len(d)
            e_items[i].out, e_items[i].out_cap = C.c_void_p(outs[i].data_ptr()), outs[i].numel()
        assert L.mi355_deflate_encode_batch_device(ctx._h, e_items, k, C.byref(opts), None) == 0
        for i in range(k):
            v_items[i].in_, v_items[i].in_len = e_items[i].in_, e_items[i].in_len
            v_items[i].out, v_items[i].out_len, v_items[i].out_cap = e_items[i].out, e_items[i].out_len, e_items[i].out_len
            i_items[i].in_, i_items[i].in_len = e_items[i].out, e_items[i].out_len  # the stream
            i_items[i].out, i_items[i].out_cap = C.c_void_p(back[i].data_ptr()), len(datas[i])

        def benc():
            assert B.mi355_deflate_encode_batch_device(bh, e_items, k, C.byref(opts), None) == 0

        def bver():
            assert B.mi355_deflate_verify_batch_device(bh, v_items, k, 0, None, None) == 0

        def binf():
            assert L.mi355_inflate_batch_device(ctx._h, i_items, k, 0, None, None) == 0
        t = alternate({"encode": benc, "verify": bver, "inflate": binf}, a.reps)
        assert all(torch.equal(back[i], ins[i]) for i in range(k))
        nbytes = sum(map(len, datas))
        res["batches"][name] = {"items": k, "bytes": nbytes, "stream_bytes": sum(e_items[i].out_len for i in range(k)),
                                "encode_ms": round(t["encode"][0], 3), "verify_ms": round(t["verify"][0], 3),
                                "verify_spread_ms": round(t["verify"][1], 3), "inflate_ms": round(t["inflate"][0], 3),
                                "inflate_spread_ms": round(t["inflate"][1], 3),
                                "inflate_over_verify": round(t["inflate"][0] / t["verify"][0], 3),
                                "inflate_over_encode": round(t["inflate"][0] / t["encode"][0], 3),
                                "inflate_gbps": round(nbytes / t["inflate"][0] / 1e6, 2)}
        del ins, outs, back

    # ---- one stream, one wave ----
    res["single"] = {}
    with open(os.path.join(ROOT, "tests", "golden", "ref_inputs", "pg11.txt"), "rb") as f:
        pg = f.read()
    rep, irep, n_out = da.VerifyReport(), da.InflateReport(), C.c_size_t(0)
    for name, data in (("pg11", pg), ("text_1MiB", datagen.text_like(1 << 20, 77))):
        d_in = dev(data)
        d_out = torch.empty(L.mi355_deflate_bound(len(data)) + 64, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(d_in.data_ptr(), len(data), d_out.data_ptr(), d_out.numel(), da.Compression.Default)
        tokens = ctx.info()["n_tokens"]
        back = torch.zeros(len(data), dtype=torch.uint8, device="cuda")

        def ver():
            assert B.mi355_deflate_verify_device(bh, C.c_void_p(d_out.data_ptr()), n, C.c_void_p(d_in.data_ptr()), len(data), 0, None, 0,
                                                 C.byref(rep), None) == 0

        def inf():
            assert L.mi355_inflate_device(ctx._h, C.c_void_p(d_out.data_ptr()), n, 0, C.c_void_p(back.data_ptr()), len(data),
                                          C.byref(n_out), C.byref(irep), None) == 0
        t = alternate({"verify": ver, "inflate": inf}, a.reps)
        assert n_out.value == len(data) and torch.equal(back, d_in)
        res["single"][name] = {"bytes": len(data), "stream_bytes": n, "tokens": tokens, "verify_ms": round(t["verify"][0], 3),
                               "inflate_ms": round(t["inflate"][0], 3), "inflate_over_verify": round(t["inflate"][0] / t["verify"][0], 3),
                               "inflate_ns_per_token": round(t["inflate"][0] * 1e6 / max(tokens, 1), 1),
                               "verify_ns_per_token": round(t["verify"][0] * 1e6 / max(tokens, 1), 1),
                               "inflate_mbps": round(len(data) / t["inflate"][0] / 1e3, 1)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
