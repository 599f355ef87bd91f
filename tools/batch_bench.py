"""tools/batch_bench.py -- the batched encode against a loop of one-input calls and against one call on the concatenation.

Device-resident inputs; --levels picks the levels (default: Default and Fast; also rle, huffman_only, best).  For each workload: (a) a loop of mi355_deflate_encode_device over the items, (b) one
mi355_deflate_encode_batch_device call, (c) one mi355_deflate_encode_device call on the concatenation of the same bytes (other
output bytes: the throughput ceiling, a yardstick only).  Every shape is warmed up before its timed window; every timed call
ends in a synchronise.  --wrapper 1 / 2 times the same workloads with zlib / gzip framing (2: the blank header, the loop over
mi355_deflate_encode_device_gzip, the batch through mi355_deflate_encode_batch_device_gzip; profiles/batch_bench_gzip.json holds
a run of 2 and of 1 from one session).  --workloads picks the workloads: by default the four of generated text, and with a level
without a hash (rle, huffman_only) also 256x64KiB_runs, rows of runs of equal bytes (the generated text has no run longer than 5).
--packed times the packed batch instead (all streams in one arena, mi355_deflate_encode_batch_packed[_device]) beside the
existing batch entries on the same workloads, the C entries called directly on prepared item arrays: device-resident packed
against mi355_deflate_encode_batch_device, and the host entries on pageable memory against each other; the runs of a pair
alternate.  Levels: Default and Fast, and RLE on the rows of runs.  Per pair the best of --reps, the baseline's spread
(max - min) and the allowance the device-resident packed call is held against: the baseline's best + two short launches
(LAUNCH_US each: kb_place and the clear) + that spread.  Per workload also packed_bound, arena_used and the input bytes.
Writes profiles/batch_bench_packed.json unless --out says otherwise.
Prints ONE JSON line.  python tools/batch_bench.py [--reps N] [--wrapper W] [--levels L,L] [--workloads W,W] [--packed] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402


LEVELS = {"default": da.Compression.Default, "fast": da.Compression.Fast, "best": da.Compression.Best,
          "rle": da.CompressionOptions.rle(), "huffman_only": da.CompressionOptions.huffman_only()}
TEXT_WORKLOADS = ("256x64KiB", "1024x4KiB", "64x1MiB", "100xpg11")
RUNS_WORKLOAD = "256x64KiB_runs"


def run_rows(n, seed, width=1024):
    """n bytes of image-like rows of `width` bytes: every row is runs of equal bytes, their lengths drawn from 1..200 (the last one
    of a row cut at its end); a run's byte is never its neighbour's, so a run is as long as it was drawn.  Seeded."""
    rnd = random.Random(seed)
    out = bytearray()
    v = rnd.randrange(256)
    while len(out) < n:
        left = width
        while left:
            r = min(rnd.randint(1, 200), left)
            v = (v + rnd.randint(1, 255)) & 255
            out += bytes([v]) * r
            left -= r
    return bytes(out[:n])


def workloads(names):
    pg = open(os.path.join(ROOT, "tests", "golden", "ref_inputs", "pg11.txt"), "rb").read()
    make = {
        "256x64KiB": lambda: [datagen.text_like(64 << 10, 1000 + k) for k in range(256)],
        "1024x4KiB": lambda: [datagen.text_like(4 << 10, 5000 + k) for k in range(1024)],
        "64x1MiB": lambda: [datagen.text_like(1 << 20, 9000 + k) for k in range(64)],
        "100xpg11": lambda: [pg] * 100,
        RUNS_WORKLOAD: lambda: [run_rows(64 << 10, 13000 + k) for k in range(256)],
    }
    return {name: make[name]() for name in names}


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


LAUNCH_US = 4.8  # a short launch such as k_plan


def packed_bench(a, ctx, L):
    """--packed: see the module's docstring"""
    w = a.wrapper
    names = [x for x in a.workloads.split(",") if x] if a.workloads else list(TEXT_WORKLOADS) + [RUNS_WORKLOAD]
    res = {"metric": "packed batch against the batch entries (best of %d, alternating runs)" % a.reps, "wrapper": w,
           "launch_us": LAUNCH_US, "workloads": {}}
    for name, datas in workloads(names).items():
        n = len(datas)
        nbytes = sum(map(len, datas))
        ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
        hlen = len(da.BLANK_GZIP_HEADER) if w == 2 else 0
        caps = [L.mi355_deflate_bound_ex(len(d), w, hlen, 0) for d in datas]
        outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for cap in caps]
        bound = da.packed_bound([len(d) for d in datas], w, None, 4)
        arena = torch.empty(bound, dtype=torch.uint8, device="cuda")
        table = torch.empty(24 * n, dtype=torch.uint8, device="cuda")
        h_outs = [(C.c_uint8 * cap)() for cap in caps]
        h_arena = (C.c_uint8 * bound)()
        torch.cuda.synchronize()
        d_items, p_items, h_items, hp_items = ((da.BatchItem * n)() for _ in range(4))
        for k, d in enumerate(datas):
            for it in (d_items, p_items):
                it[k].in_, it[k].in_len = C.c_void_p(ins[k].data_ptr()), len(d)
            for it in (h_items, hp_items):
                it[k].in_, it[k].in_len = C.cast(C.c_char_p(d), C.c_void_p), len(d)
            d_items[k].out, d_items[k].out_cap = C.c_void_p(outs[k].data_ptr()), caps[k]
            h_items[k].out, h_items[k].out_cap = C.cast(h_outs[k], C.c_void_p), caps[k]
        row = {"items": n, "bytes": nbytes, "packed_bound": bound, "item_bounds": sum(caps)}
        levels = ["default", "fast"] if name != RUNS_WORKLOAD else ["rle"]
        for lvl in levels:
            o_c = da.CompressionOptions.from_(LEVELS[lvl]).to_c(w, 0, 0)
            used = C.c_size_t(0)

            def dev_base():
                if w == 2:
                    return L.mi355_deflate_encode_batch_device_gzip(ctx._h, d_items, n, C.byref(o_c), None, 0, None)
                return L.mi355_deflate_encode_batch_device(ctx._h, d_items, n, C.byref(o_c), None)

            def dev_packed():
                return L.mi355_deflate_encode_batch_packed_device(ctx._h, p_items, n, C.byref(o_c), None, 0, C.c_void_p(arena.data_ptr()),
                                                                  bound, 4, C.c_void_p(table.data_ptr()), C.byref(used), None)

            def host_base():
                if w == 2:
                    return L.mi355_deflate_encode_batch_gzip(ctx._h, h_items, n, C.byref(o_c), None, 0)
                return L.mi355_deflate_encode_batch(ctx._h, h_items, n, C.byref(o_c))

            def host_packed():
                return L.mi355_deflate_encode_batch_packed(ctx._h, hp_items, n, C.byref(o_c), None, 0, C.cast(h_arena, C.c_void_p), bound, 4,
                                                           C.byref(used))
            fns = {"batch_device": dev_base, "packed_device": dev_packed, "batch_host": host_base, "packed_host": host_packed}
            times = {k: [] for k in fns}
            for k, fn in fns.items():  # (warm: this shape's allocations, the code objects)
                assert fn() == 0, k
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    rc = fn()
                    ms = (time.perf_counter() - t0) * 1e3  # (every entry returns after its stream has drained)
                    assert rc == 0, (k, rc)
                    times[k].append(ms)
            # the same bytes both ways, item by item
            got = arena.cpu().numpy().tobytes()
            for k in range(0, n, max(n // 16, 1)):
                off = p_items[k].out - arena.data_ptr()
                assert got[off:off + p_items[k].out_len] == outs[k][:d_items[k].out_len].cpu().numpy().tobytes(), k
                assert bytes(h_arena[hp_items[k].out - C.addressof(h_arena):][:hp_items[k].out_len]) == bytes(h_outs[k][:h_items[k].out_len]), k
            base, spread = min(times["batch_device"]), max(times["batch_device"]) - min(times["batch_device"])
            allowance = base + 2 * LAUNCH_US / 1e3 + spread
            row[lvl] = {
                "batch_device_ms": round(base, 4), "batch_device_spread_ms": round(spread, 4),
                "packed_device_ms": round(min(times["packed_device"]), 4), "allowance_ms": round(allowance, 4),
                "packed_device_within_allowance": min(times["packed_device"]) <= allowance,
                "batch_host_ms": round(min(times["batch_host"]), 4), "packed_host_ms": round(min(times["packed_host"]), 4),
                "host_batch_over_packed": round(min(times["batch_host"]) / min(times["packed_host"]), 3),
                "arena_used": used.value, "runs_ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
            }
        res["workloads"][name] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wrapper", type=int, default=0, choices=(0, 1, 2), help="0 raw, 1 zlib, 2 gzip")
    ap.add_argument("--levels", default="default,fast", help="comma-separated: " + ", ".join(LEVELS))
    ap.add_argument("--workloads", default=None, help="comma-separated: %s, %s (default: the text ones, and the runs with a level "
                    "without a hash)" % (", ".join(TEXT_WORKLOADS), RUNS_WORKLOAD))
    ap.add_argument("--out", default=None)
    ap.add_argument("--packed", action="store_true", help="the packed batch beside the batch entries (profiles/batch_bench_packed.json)")
    a = ap.parse_args()
    if a.packed:
        ctx = da.Context(0)
        res = packed_bench(a, ctx, da.load())
        ctx.close()
        line = json.dumps(res)
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "batch_bench_packed.json"), "w") as f:
            f.write(line + "\n")
        return
    levels = [x for x in a.levels.split(",") if x]
    for x in levels:
        if x not in LEVELS:
            ap.error("--levels: %r is none of %s" % (x, ", ".join(LEVELS)))
    if a.workloads:
        names = [x for x in a.workloads.split(",") if x]
        for x in names:
            if x not in TEXT_WORKLOADS + (RUNS_WORKLOAD,):
                ap.error("--workloads: %r is none of %s" % (x, ", ".join(TEXT_WORKLOADS + (RUNS_WORKLOAD,))))
    else:
        names = list(TEXT_WORKLOADS) + ([RUNS_WORKLOAD] if any(x in ("rle", "huffman_only") for x in levels) else [])
    ctx = da.Context(0)
    L = da.load()
    w = a.wrapper
    hdr = da.BLANK_GZIP_HEADER
    res = {"metric": "batched encode, device-resident (best of %d)" % a.reps, "wrapper": w, "workloads": {}}
    for name, datas in workloads(names).items():
        nbytes = sum(map(len, datas))
        ins = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
        cat = torch.cat(ins)
        outs = [torch.empty(L.mi355_deflate_bound_ex(len(d), w, len(hdr), 0), dtype=torch.uint8, device="cuda") for d in datas]
        cat_out = torch.empty(L.mi355_deflate_bound_ex(nbytes, w, len(hdr), 0) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        row = {"items": len(datas), "bytes": nbytes}
        for lvl, opt in ((x, LEVELS[x]) for x in levels):
            o_c = da.CompressionOptions.from_(opt).to_c(2, 0, 0)
            n_out = C.c_size_t(0)

            def loop():
                for x, o in zip(ins, outs):
                    if w == 2:
                        rc = L.mi355_deflate_encode_device_gzip(ctx._h, C.c_void_p(x.data_ptr()), x.numel(), C.byref(o_c), hdr, len(hdr),
                                                                C.c_void_p(o.data_ptr()), o.numel(), C.byref(n_out), None)
                        assert rc == 0, rc
                    else:
                        ctx.encode_device(x.data_ptr(), x.numel(), o.data_ptr(), o.numel(), opt, wrapper=w)

            def one_batch():
                if w == 2:
                    ctx.encode_batch_device_gzip(ins, outs, options=opt)
                else:
                    ctx.encode_batch_device(ins, outs, options=opt, wrapper=w)

            def concat():
                ctx.encode_device(cat.data_ptr(), cat.numel(), cat_out.data_ptr(), cat_out.numel(), opt, wrapper=w)
            t_loop, t_batch, t_cat = timed(loop, a.reps), timed(one_batch, a.reps), timed(concat, a.reps)
            one_batch()
            bi = ctx.batch_info()
            row[lvl] = {
                "loop_ms": round(t_loop, 3), "loop_gbps": round(nbytes / t_loop / 1e6, 3),
                "batch_ms": round(t_batch, 3), "batch_gbps": round(nbytes / t_batch / 1e6, 3),
                "concat_ms": round(t_cat, 3), "concat_gbps": round(nbytes / t_cat / 1e6, 3),
                "batch_over_loop": round(t_loop / t_batch, 2), "batch_over_concat": round(t_cat / t_batch, 3),
                "n_batched": bi["n_batched"], "n_single": bi["n_single"], "sub_batches": bi["sub_batches"],
            }
            if bi["n_spec_single"]:  # (items whose speculative parse failed in the set and that were encoded again singly)
                row[lvl]["n_spec_single"] = bi["n_spec_single"]
        res["workloads"][name] = row
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
