"""tools/inflate_seek_bench.py -- what a seek index of ONE large stream costs to build and what a byte range costs to read from it,
against the parallel inflate of the whole stream (mi355_inflate_parallel_device), which is what a caller paid for a range before.

One MI355X, device-resident data, best of --reps (default 5) with the spread beside it, the runs of a group alternating in one
session, on the 100 MB text of bench.py deflated by Python's zlib at level 6 (raw).  Every timed call returns after its stream has
drained; every range read is compared with the input once, outside the timing.
  build     mi355_inflate_seek_build_device at the default spacing against mi355_inflate_parallel_device of the same stream
  reads     single reads of 4 KiB, 64 KiB, 1 MiB and 16 MiB, each at --offsets (default 8) seeded random offsets whose times are
            summed, and one batch of 256 x 64 KiB, at point spacings of 256 KiB, 1 MiB and 4 MiB; each beside the full parallel inflate
            of the same session, with the plan's counts (entries decoded, symbols stored) of the last read of each kind
  spans     the same reads at the default spacing with the table found at MI355_CFG_INFLATE_INDEX_SPAN_BYTES = 4 KiB and 16 KiB:
            the size of a table entry is what one wave has to decode for a read
Writes profiles/inflate_seek_bench.json (--out) and prints the same JSON line.  --size N: bytes of the text (default 100 000 000)."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

SPACINGS = (256 << 10, 1 << 20, 4 << 20)
SPANS = (4 << 10, 16 << 10)
SIZES = (4 << 10, 64 << 10, 1 << 20, 16 << 20)
SPAN_DEFAULT = 16 << 10  # the default of MI355_CFG_INFLATE_INDEX_SPAN_BYTES


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
    ap.add_argument("--offsets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_seek_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    n = len(data)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    z = zlib.compress(data, 6)[2:-4]
    d_s = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_rng = torch.empty(max(max(SIZES), 256 * (64 << 10)), dtype=torch.uint8, device="cuda")
    got, irep = C.c_size_t(0), da.InflateReport()
    res = {"metric": "seek index of one stream: build and range reads (best of %d, alternating runs, device-resident, zlib -6 raw)" % a.reps,
           "device": torch.cuda.get_device_name(0), "bytes": n, "stream_bytes": len(z), "offsets_per_size": a.offsets}
    rnd = random.Random(20261019)
    sizes = [s for s in SIZES if s < n]
    offs = {s: [rnd.randrange(0, n - s) for _ in range(a.offsets)] for s in sizes}
    batch = [(rnd.randrange(0, n - (64 << 10)), 64 << 10) for _ in range(256)]

    def parallel():
        rc = L.mi355_inflate_parallel_device(ctx._h, C.c_void_p(d_s.data_ptr()), len(z), 0, C.c_void_p(d_out.data_ptr()), n, C.byref(got),
                                             C.byref(irep), None)
        assert rc == 0 and got.value == n, (rc, irep.as_dict())

    def build(spacing):
        return ctx.inflate_seek_device(d_s.data_ptr(), len(z), 0, spacing)

    def reads_of(ix):
        """the timed functions of one index, and a check of each outside the timing"""
        def single(s):
            def run():
                for off in offs[s]:
                    ix.read_device(off, s, d_rng.data_ptr(), d_s.data_ptr(), check=True)
            return run

        def many():
            ix.read_batch_device([(off, ln, d_rng.data_ptr() + k * ln) for k, (off, ln) in enumerate(batch)], d_s.data_ptr(), check=True)

        fns = {"read_%d" % s: single(s) for s in sizes}
        fns["batch_256x64k"] = many
        return fns

    def check(ix):
        for s in sizes:
            off = offs[s][-1]
            d_rng.zero_()
            ix.read_device(off, s, d_rng.data_ptr(), d_s.data_ptr(), check=True)
            assert torch.equal(d_rng[:s], d_in[off:off + s]), (s, off)
        d_rng.zero_()
        ix.read_batch_device([(off, ln, d_rng.data_ptr() + k * ln) for k, (off, ln) in enumerate(batch)], d_s.data_ptr(), check=True)
        for k in (0, 100, 255):
            off, ln = batch[k]
            assert torch.equal(d_rng[k * ln:(k + 1) * ln], d_in[off:off + ln]), k

    def measure(ix):
        fns = reads_of(ix)
        fns["parallel_full"] = parallel
        t = alternate(fns, a.reps)
        check(ix)
        r = {"points": ix.info()["n_points"], "entries": ix.info()["n_entries"], "device_bytes": ix.info()["device_bytes"]}
        for k, (best, spread) in t.items():
            per = a.offsets if k.startswith("read_") else 1
            r[k + "_ms"], r[k + "_spread_ms"] = round(best / per, 3), round(spread / per, 3)
        for s in sizes:  # what the last read of each size decoded
            ix.read_device(offs[s][-1], s, d_rng.data_ptr(), d_s.data_ptr(), check=True)
            r["read_%d_plan" % s] = ix.last_read()
        return r

    # build against the full parallel inflate
    built = []

    def build_default():
        built.append(build(0))
        if len(built) > 1:
            built.pop(0).close()

    t = alternate({"build": build_default, "parallel_full": parallel}, a.reps)
    d_out.zero_()
    parallel()
    assert torch.equal(d_out, d_in)
    res["build_ms"], res["build_spread_ms"] = round(t["build"][0], 3), round(t["build"][1], 3)
    res["parallel_full_ms"], res["parallel_full_spread_ms"] = round(t["parallel_full"][0], 3), round(t["parallel_full"][1], 3)
    res["build_over_parallel"] = round(t["build"][0] / t["parallel_full"][0], 3)
    built.pop().close()
    res["spacings"] = {}
    for spacing in SPACINGS:
        ix = build(spacing)
        res["spacings"][str(spacing)] = measure(ix)
        ix.close()
    res["spans"] = {}
    for span in SPANS:
        ctx.config(da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, span)
        ix = build(0)
        res["spans"][str(span)] = measure(ix)
        ix.close()
    ctx.config(da.Context.CFG_INFLATE_INDEX_SPAN_BYTES, SPAN_DEFAULT)
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
