"""tools/bgzf_read_bench.py -- what a member index of a BGZF file costs to build and what a byte range of the uncompressed data costs
to read through it (mi355_bgzf_index_build_device, mi355_bgzf_read*), against the members inflate of the whole file
(mi355_inflate_members_device), which is what a caller paid for a range before, and against a seek read with 4 KiB cuts of the same
text as ONE gzip member.

One MI355X, medians of --reps (default 5) with the spread (max - min) beside them, the runs of a group alternating in one session, on
the 100 MB text of bench.py as the library's own BGZF file (mi355_bgzf_encode_device) at the default block size and at block 4096.
Every timed call returns after its stream has drained; every read is compared with the input once, outside the timing; every ratio
is taken against a figure of the same group.
  index     mi355_bgzf_index_build_device beside the members inflate of the file
  reads     single reads of 4 KiB, 64 KiB, 1 MiB, 16 MiB at --offsets (default 8) seeded random offsets whose times are summed, the
            whole file, and batches of 256 x 64 KiB and 4096 x 4 KiB, device resident; with the plan's counts of the last read of
            each kind, the library's own clock (report.ms) of one more run of each batch, and -- from a second pass with the stage
            clocks on -- the milliseconds per launch kind
  host      the same single reads and the whole file through mi355_bgzf_read on host bytes, with the compressed bytes it copied
  seek      single reads of the same sizes through a seek index with 4 KiB cuts of the text as one gzip member
Writes profiles/bgzf_read_bench.json (--out) and prints the same JSON line.  --size N: bytes of the text (default 100 000 000)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

BLOCKS = (0, 4096)
SIZES = (4 << 10, 64 << 10, 1 << 20, 16 << 20)
BATCHES = ((256, 64 << 10), (4096, 4 << 10))


def alternate(fns, reps):
    """every function once to warm, then reps rounds in turn: {name: (median ms, spread ms)}"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--offsets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_read_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    n = len(data)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    res = {"metric": "BGZF reads: member index and byte ranges (median of %d with max - min, alternating runs, one MI355X)" % a.reps,
           "device": torch.cuda.get_device_name(0), "bytes": n, "offsets_per_size": a.offsets, "blocks": {}}
    rnd = random.Random(20261021)
    sizes = [s for s in SIZES if s < n]
    offs = {s: [rnd.randrange(0, n - s) for _ in range(a.offsets)] for s in sizes}
    batches = {"batch_%dx%dk" % (k, s >> 10): [(rnd.randrange(0, n - s), s) for _ in range(k)] for k, s in BATCHES if s < n}
    got, nm, irep = C.c_size_t(0), C.c_size_t(0), da.InflateReport()

    def put(r, t, per_of):
        for k, (med, spread) in t.items():
            per = per_of(k)
            r[k + "_ms"], r[k + "_spread_ms"] = round(med / per, 4), round(spread / per, 4)

    for block in BLOCKS:
        cap = da.bgzf_bound(n, block)
        d_file = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
        _rc, flen, n_members, _m = ctx.encode_bgzf_device(d_in.data_ptr(), n, d_file.data_ptr(), cap, block_size=block, room=0)
        file = d_file[:flen].cpu().numpy().tobytes()
        r = {"file_bytes": flen, "members": n_members}

        def members_full():
            rc = L.mi355_inflate_members_device(ctx._h, C.c_void_p(d_file.data_ptr()), flen, C.c_void_p(d_out.data_ptr()), n, C.byref(got), None, 0,
                                                C.byref(nm), C.byref(irep), None)
            assert rc == 0 and got.value == n, (rc, irep.as_dict())

        # ---- the index build ----
        built = []

        def build():
            built.append(ctx.bgzf_index_device(d_file.data_ptr(), flen))
            if len(built) > 1:
                built.pop(0).close()

        t = alternate({"index_build": build, "members_full": members_full}, a.reps)
        put(r, t, lambda k: 1)
        r["index_build_over_members_full"] = round(t["index_build"][0] / t["members_full"][0], 4)
        ix = built.pop()
        r["index_host_bytes"] = ix.info()["host_bytes"]
        d_out.zero_()
        members_full()
        assert torch.equal(d_out[:n], d_in)

        # ---- device-resident reads ----
        def single(s):
            def run():
                for off in offs[s]:
                    ix.read_device(off, s, d_out.data_ptr(), check=True)
            return run

        def whole():
            ix.read_device(0, n, d_out.data_ptr(), check=True)

        def many(rs):
            def run():
                at, items = 0, []
                for off, ln in rs:
                    items.append((off, ln, d_out.data_ptr() + at))
                    at += ln
                ix.read_batch_device(items, check=True)
            return run

        fns = {"read_%d" % s: single(s) for s in sizes}
        fns["read_whole"] = whole
        for k, rs in batches.items():
            fns[k] = many(rs)
        fns["members_full"] = members_full
        t = alternate(fns, a.reps)
        dev = {}
        put(dev, t, lambda k: a.offsets if k.startswith("read_") and k != "read_whole" else 1)
        for k in fns:
            if k != "members_full":
                dev[k + "_over_members_full"] = round(dev[k + "_ms"] / dev["members_full_ms"], 4)
        # a batch's time above holds this binding's bookkeeping of its ranges (lists, ctypes arrays, a dict per report): beside it
        # the library's own host clock around the call, report.ms, of one more run
        for k, rs in batches.items():
            at, items = 0, []
            for off, ln in rs:
                items.append((off, ln, d_out.data_ptr() + at))
                at += ln
            dev[k + "_library_ms"] = round(ix.read_batch_device(items, check=True)[1][0][2]["ms"], 4)
        # the checks, the plan's counts and the launch kinds, outside the timing
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
        for s in sizes:
            off = offs[s][-1]
            d_out.zero_()
            ix.read_device(off, s, d_out.data_ptr(), check=True)
            assert torch.equal(d_out[:s], d_in[off:off + s]), (block, s, off)
            dev["read_%d_plan" % s] = ix.last_read()
            dev["read_%d_stages_ms" % s] = {k: round(v, 4) for k, v in ctx.bgzf_last_read_stages().items()}
        d_out.zero_()
        whole()
        assert torch.equal(d_out[:n], d_in), block
        dev["read_whole_plan"] = ix.last_read()
        dev["read_whole_stages_ms"] = {k: round(v, 4) for k, v in ctx.bgzf_last_read_stages().items()}
        for k, rs in batches.items():
            d_out.zero_()
            many(rs)()
            at = 0
            for j, (off, ln) in enumerate(rs):
                if j % 97 == 0:
                    assert torch.equal(d_out[at:at + ln], d_in[off:off + ln]), (block, k, j)
                at += ln
            dev[k + "_plan"] = ix.last_read()
            dev[k + "_stages_ms"] = {kk: round(v, 4) for kk, v in ctx.bgzf_last_read_stages().items()}
        ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
        r["device"] = dev

        # ---- the same reads through the host form ----
        hix = da.bgzf_index_from_members(ix.members(), flen)

        def host_single(s):
            def run():
                for off in offs[s]:
                    hix.read_raw(off, s, ctx=ctx, file=file)
            return run

        hf = {"read_%d" % s: host_single(s) for s in sizes}
        hf["read_whole"] = lambda: hix.read_raw(0, n, ctx=ctx, file=file)
        hf["members_full"] = members_full
        t = alternate(hf, a.reps)
        host = {}
        put(host, t, lambda k: a.offsets if k.startswith("read_") and k != "read_whole" else 1)
        for s in sizes:
            rc, g, _rep, back = hix.read_raw(offs[s][-1], s, ctx=ctx, file=file)
            assert rc == 0 and back == data[offs[s][-1]:offs[s][-1] + s]
            host["read_%d_copied_bytes" % s] = hix.last_read(ctx)["copied"]
        rc, g, _rep, back = hix.read_raw(0, n, ctx=ctx, file=file)
        assert rc == 0 and back == data
        host["read_whole_copied_bytes"] = hix.last_read(ctx)["copied"]
        r["host"] = host
        hix.close()
        ix.close()
        res["blocks"][str(block or 65280)] = r
        del d_file

    # ---- a seek index with 4 KiB cuts of the same text as one gzip member, beside the members inflate of the default-block file ----
    z = ctx.encode_gzip(data)
    d_z = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    sx = ctx.inflate_seek_device(d_z.data_ptr(), len(z), 2, 0, cut=4096)
    cap = da.bgzf_bound(n, 0)
    d_file = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    _rc, flen, _nm, _m = ctx.encode_bgzf_device(d_in.data_ptr(), n, d_file.data_ptr(), cap, room=0)
    bx = ctx.bgzf_index_device(d_file.data_ptr(), flen)

    def seek_single(s):
        def run():
            for off in offs[s]:
                sx.read_device(off, s, d_out.data_ptr(), d_z.data_ptr(), check=True)
        return run

    def bgzf_single(s):
        def run():
            for off in offs[s]:
                bx.read_device(off, s, d_out.data_ptr(), check=True)
        return run

    fns = {}
    for s in sizes:
        fns["seek_%d" % s] = seek_single(s)
        fns["bgzf_%d" % s] = bgzf_single(s)
    t = alternate(fns, a.reps)
    seek = {"gzip_bytes": len(z), "cut_bytes": 4096, "cuts": sx.cut_info()["n_cuts"], "points": sx.info()["n_points"]}
    put(seek, t, lambda k: a.offsets)
    for s in sizes:
        seek["bgzf_over_seek_%d" % s] = round(seek["bgzf_%d_ms" % s] / seek["seek_%d_ms" % s], 4)
        d_out.zero_()
        sx.read_device(offs[s][-1], s, d_out.data_ptr(), d_z.data_ptr(), check=True)
        assert torch.equal(d_out[:s], d_in[offs[s][-1]:offs[s][-1] + s])
    res["seek_4k_cuts"] = seek
    sx.close()
    bx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
