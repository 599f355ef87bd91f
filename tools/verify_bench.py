"""tools/verify_bench.py -- what the verify entry points cost, against the encodes they check.

One MI355X, device-resident data, best of --reps (default 5), the runs of a pair alternating in one session:
  text100   the 100 MB text of bench.py at Default: mi355_deflate_verify_device with the encode's block table (a wave per
            block) against mi355_deflate_encode_device of the baseline library
  tableless mi355_deflate_verify_device without a table (ONE wave walks the stream) on pg11.txt and on 1 MiB of text
  batches   mi355_deflate_verify_batch_device on 256 x 64 KiB and 1024 x 4 KiB against the baseline's
            mi355_deflate_encode_batch_device of the same items
The baseline library is the file MI355_BASELINE_LIB names (a build of the parent commit: `make -C deflate-rs_amd` in a
checkout of it) and this tree's own library when the variable is not set -- the encode path is the same text either way, and the
result says which it was.  Every timed call returns after its stream has drained.
Writes profiles/verify_bench.json (--out) and prints the same JSON line.  --size N: bytes of the large text (default 100 000 000)."""
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
    """(the library the encodes are timed on, a context of it, what it is)"""
    path = os.environ.get("MI355_BASELINE_LIB", "")
    if not path:
        return da.load(), None, "this tree's library"
    B = C.CDLL(path)
    B.mi355_deflate_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    B.mi355_deflate_ctx_destroy.argtypes = [C.c_void_p]
    B.mi355_deflate_ctx_destroy.restype = None
    B.mi355_deflate_encode_device.argtypes = da.load().mi355_deflate_encode_device.argtypes
    B.mi355_deflate_encode_batch_device.argtypes = da.load().mi355_deflate_encode_batch_device.argtypes
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    B, bh, which = baseline_library()
    bh = bh or ctx._h
    opts = da.CompressionOptions.from_(da.Compression.Default).to_c(0, 0, 0)
    res = {"metric": "verify against the encode it checks (best of %d, alternating runs, device-resident)" % a.reps,
           "baseline": which, "device": torch.cuda.get_device_name(0)}

    def encode_with_table(data):
        d_in = dev(data)
        d_out = torch.empty(L.mi355_deflate_bound(len(data)) + 64, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(d_in.data_ptr(), len(data), d_out.data_ptr(), d_out.numel(), da.Compression.Default)
        blocks = ctx.blocks()
        arr, nb = ctx._block_table(blocks)
        return d_in, d_out, n, arr, nb

    # ---- the large text, with the table ----
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    d_in, d_out, n, arr, nb = encode_with_table(data)
    base_out = torch.empty_like(d_out)
    n_out = C.c_size_t(0)
    rep = da.VerifyReport()

    def enc():
        rc = B.mi355_deflate_encode_device(bh, C.c_void_p(d_in.data_ptr()), len(data), C.byref(opts), C.c_void_p(base_out.data_ptr()),
                                           base_out.numel(), C.byref(n_out), None)
        assert rc == 0, rc

    def ver():
        rc = L.mi355_deflate_verify_device(ctx._h, C.c_void_p(d_out.data_ptr()), n, C.c_void_p(d_in.data_ptr()), len(data), 0, arr, nb,
                                           C.byref(rep), None)
        assert rc == 0, (rc, rep.as_dict())
    t = alternate({"encode": enc, "verify": ver}, a.reps)
    assert n_out.value == n
    res["text100"] = {"bytes": len(data), "stream_bytes": n, "entries": nb, "deflate_blocks": rep.n_blocks,
                      "encode_ms": round(t["encode"][0], 3), "encode_spread_ms": round(t["encode"][1], 3),
                      "verify_ms": round(t["verify"][0], 3), "verify_spread_ms": round(t["verify"][1], 3),
                      "verify_over_encode": round(t["verify"][0] / t["encode"][0], 3),
                      "verify_gbps": round(len(data) / t["verify"][0] / 1e6, 2)}
    del d_in, d_out, base_out

    # ---- one wave, no table ----
    res["tableless"] = {}
    with open(os.path.join(ROOT, "tests", "golden", "ref_inputs", "pg11.txt"), "rb") as f:
        pg = f.read()
    for name, data in (("pg11", pg), ("text_1MiB", datagen.text_like(1 << 20, 77))):
        d_in, d_out, n, arr, nb = encode_with_table(data)

        def tabled():
            assert L.mi355_deflate_verify_device(ctx._h, C.c_void_p(d_out.data_ptr()), n, C.c_void_p(d_in.data_ptr()), len(data), 0, arr,
                                                 nb, C.byref(rep), None) == 0

        def tableless():
            assert L.mi355_deflate_verify_device(ctx._h, C.c_void_p(d_out.data_ptr()), n, C.c_void_p(d_in.data_ptr()), len(data), 0, None,
                                                 0, C.byref(rep), None) == 0
        t = alternate({"tabled": tabled, "tableless": tableless}, a.reps)
        tokens = ctx.info()["n_tokens"]
        res["tableless"][name] = {"bytes": len(data), "stream_bytes": n, "entries": nb, "tokens": tokens,
                                  "tableless_ms": round(t["tableless"][0], 3), "tabled_ms": round(t["tabled"][0], 3),
                                  "tableless_ns_per_token": round(t["tableless"][0] * 1e6 / max(tokens, 1), 1),
                                  "tableless_mbps": round(len(data) / t["tableless"][0] / 1e3, 1)}

    # ---- batches ----
    res["batches"] = {}
    for name, datas in (("256x64KiB", [datagen.text_like(64 << 10, 1000 + k) for k in range(256)]),
                        ("1024x4KiB", [datagen.text_like(4 << 10, 5000 + k) for k in range(1024)])):
        k = len(datas)
        ins = [dev(d) for d in datas]
        outs = [torch.empty(L.mi355_deflate_bound_ex(len(d), 0, 0, 0), dtype=torch.uint8, device="cuda") for d in datas]
        e_items, v_items = (da.BatchItem * k)(), (da.BatchItem * k)()
        for i, d in enumerate(datas):
            e_items[i].in_, e_items[i].in_len = C.c_void_p(ins[i].data_ptr()), len(d)
            e_items[i].out, e_items[i].out_cap = C.c_void_p(outs[i].data_ptr()), outs[i].numel()
        assert L.mi355_deflate_encode_batch_device(ctx._h, e_items, k, C.byref(opts), None) == 0
        for i in range(k):
            v_items[i].in_, v_items[i].in_len = e_items[i].in_, e_items[i].in_len
            v_items[i].out, v_items[i].out_len, v_items[i].out_cap = e_items[i].out, e_items[i].out_len, e_items[i].out_len

        def benc():
            assert B.mi355_deflate_encode_batch_device(bh, e_items, k, C.byref(opts), None) == 0

        def bver():
            assert L.mi355_deflate_verify_batch_device(ctx._h, v_items, k, 0, None, None) == 0
        t = alternate({"encode": benc, "verify": bver}, a.reps)
        nbytes = sum(map(len, datas))
        res["batches"][name] = {"items": k, "bytes": nbytes, "encode_ms": round(t["encode"][0], 3), "verify_ms": round(t["verify"][0], 3),
                                "verify_spread_ms": round(t["verify"][1], 3), "verify_over_encode": round(t["verify"][0] / t["encode"][0], 3),
                                "verify_gbps": round(nbytes / t["verify"][0] / 1e6, 2)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
