"""tools/batch_bench.py -- the batched encode against a loop of one-input calls and against one call on the concatenation.

Device-resident inputs, Default and Fast.  For each workload: (a) a loop of mi355_deflate_encode_device over the items, (b) one
mi355_deflate_encode_batch_device call, (c) one mi355_deflate_encode_device call on the concatenation of the same bytes (other
output bytes: the throughput ceiling, a yardstick only).  Every shape is warmed up before its timed window; every timed call
ends in a synchronise.  Prints ONE JSON line.  python tools/batch_bench.py [--reps N] [--out FILE]"""
import argparse
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


def workloads():
    pg = open(os.path.join(ROOT, "tests", "golden", "ref_inputs", "pg11.txt"), "rb").read()
    return {
        "256x64KiB": [datagen.text_like(64 << 10, 1000 + k) for k in range(256)],
        "1024x4KiB": [datagen.text_like(4 << 10, 5000 + k) for k in range(1024)],
        "64x1MiB": [datagen.text_like(1 << 20, 9000 + k) for k in range(64)],
        "100xpg11": [pg] * 100,
    }


def timed(fn, reps):
    fn()  # (warm: this shape's allocations, the code objects)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None or ms < best else best
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = da.Context(0)
    L = da.load()
    res = {"metric": "batched encode, device-resident (best of %d)" % a.reps, "workloads": {}}
    for name, datas in workloads().items():
        nbytes = sum(map(len, datas))
        ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
        cat = torch.cat(ins)
        outs = [torch.empty(L.mi355_deflate_bound_ex(len(d), 0, 0, 0), dtype=torch.uint8, device="cuda") for d in datas]
        cat_out = torch.empty(L.mi355_deflate_bound_ex(nbytes, 0, 0, 0) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        row = {"items": len(datas), "bytes": nbytes}
        for lvl, opt in (("default", da.Compression.Default), ("fast", da.Compression.Fast)):
            def loop():
                for x, o in zip(ins, outs):
                    ctx.encode_device(x.data_ptr(), x.numel(), o.data_ptr(), o.numel(), opt)

            def one_batch():
                ctx.encode_batch_device(ins, outs, options=opt)

            def concat():
                ctx.encode_device(cat.data_ptr(), cat.numel(), cat_out.data_ptr(), cat_out.numel(), opt)
            t_loop, t_batch, t_cat = timed(loop, a.reps), timed(one_batch, a.reps), timed(concat, a.reps)
            ctx.encode_batch_device(ins, outs, options=opt)
            bi = ctx.batch_info()
            row[lvl] = {
                "loop_ms": round(t_loop, 3), "loop_gbps": round(nbytes / t_loop / 1e6, 3),
                "batch_ms": round(t_batch, 3), "batch_gbps": round(nbytes / t_batch / 1e6, 3),
                "concat_ms": round(t_cat, 3), "concat_gbps": round(nbytes / t_cat / 1e6, 3),
                "batch_over_loop": round(t_loop / t_batch, 2), "batch_over_concat": round(t_cat / t_batch, 3),
                "n_batched": bi["n_batched"], "n_single": bi["n_single"], "sub_batches": bi["sub_batches"],
            }
        res["workloads"][name] = row
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
