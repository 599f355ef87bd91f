"""tools/inflate_cut_bench.py -- what cuts inside the table entries of a seek index (MI355_CFG_INFLATE_SEEK_CUT_BYTES) cost at the
build and save at a read.

The workload and the timing method are tools/inflate_seek_bench.py's: one MI355X, device-resident data, best of --reps (default 5)
with the spread beside it, on the 100 MB text of bench.py deflated by Python's zlib at level 6 (raw), the default point spacing.
The runs of a group ALTERNATE over the cut sizes in one session, cut_bytes = 0 among them: that is the path without cuts, and the
baseline of every ratio here is that run and no older figure.  Every timed call returns after its stream has drained; every range
read is compared with the input once, outside the timing.
  build     mi355_inflate_seek_build_device at cut_bytes = 0, 1 KiB, 4 KiB, 16 KiB and 64 KiB; the cuts and the host bytes they take
  reads     single reads of 4 KiB, 64 KiB, 1 MiB and 16 MiB, each at --offsets (default 8) seeded random offsets whose times are
            summed, and one batch of 256 x 64 KiB; with what the last read of each kind decoded (last_read_cuts)
  single    the same reads on --single-size bytes (default 10 000 000) of the text as zlib -0 (stored blocks) and as Z_FIXED: with
            cuts off each is ONE entry and a read costs the whole lead-in to one wave, so these run at --single-offsets (default 2)
            offsets and --single-reps (default 3)
  stages    per cut size and read kind, the HIP-event time per launch kind -- pass 1 (entries or cuts), flatten, windows, resolve --
            from one more run of the same reads with MI355_CFG_STAGE_CLOCKS on (mi355_inflate_seek_last_read_stages), outside the
            latency figures: an event is idle queue between two kernels
  walker    the build at cut_bytes = 4 KiB with MI355_CFG_INFLATE_SEEK_CUT_WALKER = 1 -- pass 1 as without cuts, the cuts from a second
            launch that stores no symbol -- alternating with the builds that record the cuts in pass 1
Writes profiles/inflate_cut_bench.json (--out) and prints the same JSON line."""
import argparse
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

CUTS = (0, 1 << 10, 4 << 10, 16 << 10, 64 << 10)
SIZES = (4 << 10, 64 << 10, 1 << 20, 16 << 20)
WALKER_CUT = 4 << 10


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


def sweep(ctx, data, z, reps, n_offsets, seed, batch_n):
    """one stream at every cut size: {"build": ..., "cuts": {cut_bytes: ...}}"""
    n = len(data)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_s = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    sizes = [s for s in SIZES if s < n]
    d_rng = torch.empty(max(max(sizes), batch_n * (64 << 10)), dtype=torch.uint8, device="cuda")
    rnd = random.Random(seed)
    offs = {s: [rnd.randrange(0, n - s) for _ in range(n_offsets)] for s in sizes}
    batch = [(rnd.randrange(0, n - (64 << 10)), 64 << 10) for _ in range(batch_n)]
    print("%d bytes from %d" % (n, len(z)), file=sys.stderr, flush=True)
    out = {"bytes": n, "stream_bytes": len(z), "offsets_per_size": n_offsets, "reps": reps, "batch": "%dx64k" % batch_n, "cuts": {}}

    # the build, the cut sizes alternating
    built = {}

    def build_at(cut):
        def run():
            if cut in built:
                built.pop(cut).close()
            built[cut] = ctx.inflate_seek_device(d_s.data_ptr(), len(z), 0, 0, cut=cut)
        return run

    def build_walker():
        ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_WALKER, 1)
        try:
            build_at(WALKER_CUT)()
        finally:
            ctx.config(da.Context.CFG_INFLATE_SEEK_CUT_WALKER, 0)

    fns = {cut: build_at(cut) for cut in CUTS}
    fns["walker"] = build_walker
    fns["last"] = build_at(WALKER_CUT)  # (so that the handle kept for the reads is one that recorded its cuts in pass 1)
    t = alternate(fns, reps)
    out["walker"] = {"cut_bytes": WALKER_CUT, "build_ms": round(t["walker"][0], 3), "build_spread_ms": round(t["walker"][1], 3),
                     "build_over_no_cuts": round(t["walker"][0] / t[0][0], 3), "build_over_recording": round(t["walker"][0] / t[WALKER_CUT][0], 3)}
    for cut in CUTS:
        ix = built[cut]
        info = ix.cut_info()
        out["cuts"][str(cut)] = {"build_ms": round(t[cut][0], 3), "build_spread_ms": round(t[cut][1], 3),
                                 "build_over_no_cuts": round(t[cut][0] / t[0][0], 3), "n_cuts": info["n_cuts"], "host_bytes": info["host_bytes"],
                                 "largest_cut": info["largest_cut"], "entries": ix.info()["n_entries"], "points": ix.info()["n_points"]}

    def single(ix, s):
        def run():
            for off in offs[s]:
                ix.read_device(off, s, d_rng.data_ptr(), d_s.data_ptr(), check=True)
        return run

    def many(ix):
        def run():
            ix.read_batch_device([(off, ln, d_rng.data_ptr() + k * ln) for k, (off, ln) in enumerate(batch)], d_s.data_ptr(), check=True)
        return run

    def stages(fn, per):
        """the launch kinds' milliseconds of one more run of fn with the stage clocks on, per read"""
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
        try:
            total = dict(pass1=0.0, flatten=0.0, windows=0.0, resolve=0.0)
            for one in fn:
                one()
                for k, v in ctx.inflate_seek_last_read_stages().items():
                    total[k] += v
        finally:
            ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
        return {k: round(v / per, 3) for k, v in total.items()}

    # a read kind at a time, the cut sizes alternating
    for s in sizes:
        t = alternate({cut: single(built[cut], s) for cut in CUTS}, reps)
        for cut in CUTS:
            r = out["cuts"][str(cut)]
            r["read_%d_ms" % s], r["read_%d_spread_ms" % s] = round(t[cut][0] / n_offsets, 3), round(t[cut][1] / n_offsets, 3)
            r["read_%d_over_no_cuts" % s] = round(t[cut][0] / t[0][0], 3)
            ix = built[cut]
            d_rng.zero_()
            ix.read_device(offs[s][-1], s, d_rng.data_ptr(), d_s.data_ptr(), check=True)
            assert torch.equal(d_rng[:s], d_in[offs[s][-1]:offs[s][-1] + s]), (cut, s)
            r["read_%d_did" % s] = dict(ix.last_read_cuts(), entries=ix.last_read()["entries"])
            r["read_%d_stages_ms" % s] = stages([(lambda off=off: ix.read_device(off, s, d_rng.data_ptr(), d_s.data_ptr(), check=True))
                                                 for off in offs[s]], n_offsets)
    t = alternate({cut: many(built[cut]) for cut in CUTS}, reps)
    for cut in CUTS:
        r = out["cuts"][str(cut)]
        r["batch_ms"], r["batch_spread_ms"], r["batch_over_no_cuts"] = round(t[cut][0], 3), round(t[cut][1], 3), round(t[cut][0] / t[0][0], 3)
        d_rng.zero_()
        many(built[cut])()
        for k in (0, batch_n // 2, batch_n - 1):
            off, ln = batch[k]
            assert torch.equal(d_rng[k * ln:(k + 1) * ln], d_in[off:off + ln]), (cut, k)
        r["batch_did"] = dict(built[cut].last_read_cuts(), entries=built[cut].last_read()["entries"])
        r["batch_stages_ms"] = stages([many(built[cut])], 1)
    for ix in built.values():
        ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--offsets", type=int, default=8)
    ap.add_argument("--single-size", type=int, default=10_000_000)
    ap.add_argument("--single-reps", type=int, default=3)
    ap.add_argument("--single-offsets", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_cut_bench.json"))
    a = ap.parse_args()
    ctx = da.Context(0)
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    res = {"metric": "cuts inside the entries of a seek index: build and range reads per cut_bytes (best of reps, the cut sizes alternating, "
                     "cut_bytes 0 = no cuts in the same run, device-resident, default spacing)",
           "device": torch.cuda.get_device_name(0), "cut_bytes": list(CUTS)}
    res["zlib6"] = sweep(ctx, data, zlib.compress(data, 6)[2:-4], a.reps, a.offsets, 20261020, 256)
    small = data[:a.single_size]
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    res["zlib0_stored"] = sweep(ctx, small, c.compress(small) + c.flush(), a.single_reps, a.single_offsets, 20261021, 32)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    res["zfixed"] = sweep(ctx, small, c.compress(small) + c.flush(), a.single_reps, a.single_offsets, 20261022, 32)
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
