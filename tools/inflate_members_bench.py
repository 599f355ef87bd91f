"""tools/inflate_members_bench.py -- what the inflate of a gzip FILE of many members costs (mi355_inflate_members_device), against
the same decode without the discovery and against the parallel inflate of the same text as one member.

One MI355X, device-resident data, best of --reps (default 5), the runs of a group alternating in one session, on the 100 MB text of
bench.py as bgzip would cut it: blocks of 0xff00 bytes deflated by Python's zlib at level 6, each a member with a 'BC' subfield, and
the 28-byte end-of-file marker.
  members   mi355_inflate_members_device on the BGZF file
  stages    the same call with MI355_CFG_STAGE_CLOCKS on, a context of its own: find, walk, fill, member decode, chain decode, checksums
  sweep     the call at MI355_CFG_INFLATE_MEMBER_SPAN_BYTES = 16 KiB .. 1 MiB, alternating; which span size wins
  batch     mi355_inflate_batch_device handed the true member table from the host: the same decode without discovery
  parallel  mi355_inflate_parallel_device on the same text as ONE gzip member (zlib level 6)
  cat       mi355_inflate_members_device on a `cat` of 64, 8 and 512 plain members of the same text (--cat 0 leaves it out): the call
            with MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES at its default against mi355_inflate_parallel_device on the one member,
            alternating; its counters (mi355_inflate_members_last_parallel) and, from a context with the stage clocks on, its
            milliseconds per launch kind; and, on the 64 members, the same call with the setting at 0 -- the one wave, run once
  stored    the same 64 members as STORED blocks (zlib level 0), which one wave copies fast: the call with the setting at its default
            and at 0, alternating -- where the parallel path's fixed cost per member shows against the cheapest members there are
Every timed call returns after its stream has drained; every output is compared with the input once, outside the timing.
Writes profiles/inflate_members_bench.json (--out) and prints the same JSON line.  --size N: bytes of the text (default 100 000 000)."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

SWEEP = tuple(16 << (10 + k) for k in range(7))  # 16 KiB .. 1 MiB
SPAN_DEFAULT = 64 << 10                          # the default of MI355_CFG_INFLATE_MEMBER_SPAN_BYTES
PARALLEL_DEFAULT = 64 << 10                      # the default of MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES
BLOCK = 0xff00
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def bgzf_member(data):
    raw = raw_deflate(data)
    total = 18 + len(raw) + 8
    assert total <= 65536
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b"BC\x02\x00" + struct.pack("<H", total - 1) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def plain_member(data, level=6):
    return (bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff]) + raw_deflate(data, level) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF))


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
    ap.add_argument("--cat", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_members_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    res = {"metric": "inflate of a gzip file of many members (best of %d, alternating runs, device-resident)" % a.reps,
           "device": torch.cuda.get_device_name(0)}
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    d_in = dev(data)
    d_out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    got, nm, irep = C.c_size_t(0), C.c_size_t(0), da.InflateReport()
    parts = [bgzf_member(data[o: o + BLOCK]) for o in range(0, len(data), BLOCK)] + [BGZF_EOF]
    d_file = dev(b"".join(parts))
    file_len = sum(map(len, parts))
    one = plain_member(data)
    d_one = dev(one)

    def members(d_s, n, h=None):
        rc = L.mi355_inflate_members_device(h or ctx._h, C.c_void_p(d_s.data_ptr()), n, C.c_void_p(d_out.data_ptr()), len(data), C.byref(got),
                                            None, 0, C.byref(nm), C.byref(irep), None)
        assert rc == 0 and got.value == len(data), (rc, irep.as_dict())

    # the true member table, from the host: the batch's items
    items = (da.BatchItem * len(parts))()
    o = p = 0
    for k, part in enumerate(parts):
        size = min(BLOCK, len(data) - p) if k + 1 < len(parts) else 0
        items[k].in_, items[k].in_len = C.c_void_p(d_file.data_ptr() + o), len(part)
        items[k].out, items[k].out_cap = C.c_void_p(d_out.data_ptr() + p), size
        o, p = o + len(part), p + size

    def batch():
        for k in range(len(parts)):
            items[k].status = 0
        rc = L.mi355_inflate_batch_device(ctx._h, items, len(parts), 2, None, None)
        assert rc == 0, rc

    def parallel():
        rc = L.mi355_inflate_parallel_device(ctx._h, C.c_void_p(d_one.data_ptr()), len(one), 2, C.c_void_p(d_out.data_ptr()), len(data),
                                             C.byref(got), C.byref(irep), None)
        assert rc == 0 and got.value == len(data), (rc, irep.as_dict())

    def check(fn):  # outside the timing: the bytes
        d_out.zero_()
        fn()
        assert torch.equal(d_out, d_in)

    fns = {"members": lambda: members(d_file, file_len), "batch_with_the_table": batch, "parallel_one_member": parallel}
    t = alternate(fns, a.reps)
    for fn in fns.values():
        check(fn)
    r = {"bytes": len(data), "file_bytes": file_len, "members": len(parts), "span_bytes": SPAN_DEFAULT}
    for k, (best, spread) in t.items():
        r[k + "_ms"], r[k + "_spread_ms"] = round(best, 3), round(spread, 3)
    r["members_gbps"] = round(len(data) / t["members"][0] / 1e6, 2)
    r["members_over_batch"] = round(t["members"][0] / t["batch_with_the_table"][0], 3)
    # per launch kind: a context with the stage clocks on
    clk = da.Context(0)
    clk.config(da.Context.CFG_STAGE_CLOCKS, 1)
    rows = []
    for _ in range(a.reps + 1):
        members(d_file, file_len, clk._h)
        rows.append(clk.inflate_members_stages())
    r["stages"] = {k: round(min(row[k] for row in rows[1:]), 3) for k in rows[0]}
    clk.close()

    # the span size
    def at(S):
        def run():
            ctx.config(da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, S)
            members(d_file, file_len)
        return run
    sweep = alternate({S: at(S) for S in SWEEP}, a.reps)
    for S in SWEEP:
        check(at(S))
    ctx.config(da.Context.CFG_INFLATE_MEMBER_SPAN_BYTES, SPAN_DEFAULT)
    r["sweep"] = {str(S): {"ms": round(sweep[S][0], 3), "spread_ms": round(sweep[S][1], 3)} for S in SWEEP}
    r["sweep_best_span_bytes"] = min(SWEEP, key=lambda S: sweep[S][0])
    res["bgzf"] = r
    for k in (64, 8, 512) if a.cat else ():
        step = (len(data) + k - 1) // k
        cat = b"".join(plain_member(data[o: o + step]) for o in range(0, len(data), step))
        d_cat = dev(cat)
        fns = {"members": lambda: members(d_cat, len(cat)), "parallel_one_member": parallel}
        t = alternate(fns, a.reps)
        for fn in fns.values():
            check(fn)
        members(d_cat, len(cat))
        assert nm.value == k
        r = {"file_bytes": len(cat), "members": nm.value, "parallel_bytes": PARALLEL_DEFAULT, "ms": round(t["members"][0], 3),
             "spread_ms": round(t["members"][1], 3), "gbps": round(len(data) / t["members"][0] / 1e6, 3),
             "parallel_one_member_ms": round(t["parallel_one_member"][0], 3),
             "over_one_member": round(t["members"][0] / t["parallel_one_member"][0], 3), "counters": ctx.inflate_members_last_parallel()}
        clk = da.Context(0)
        clk.config(da.Context.CFG_STAGE_CLOCKS, 1)
        rows = []
        for _ in range(a.reps + 1):
            members(d_cat, len(cat), clk._h)
            rows.append(dict(clk.inflate_members_stages(), **clk.inflate_members_parallel_stages()))
        r["stages"] = {name: round(min(row[name] for row in rows[1:]), 3) for name in rows[0]}
        clk.close()
        if k == 64:  # the setting at 0: every member by the one wave, once
            ctx.config(da.Context.CFG_INFLATE_MEMBER_PARALLEL_BYTES, 0)
            d_out.zero_()
            t0 = time.perf_counter()
            members(d_cat, len(cat))
            ms = (time.perf_counter() - t0) * 1e3
            ctx.config(da.Context.CFG_INFLATE_MEMBER_PARALLEL_BYTES, PARALLEL_DEFAULT)
            assert torch.equal(d_out, d_in) and nm.value == k and not any(ctx.inflate_members_last_parallel().values())
            r["off_ms"], r["off_gbps"] = round(ms, 1), round(len(data) / ms / 1e6, 3)
        res["cat_%d_plain_members" % k] = r
    if a.cat:
        step = (len(data) + 63) // 64
        cat = b"".join(plain_member(data[o: o + step], 0) for o in range(0, len(data), step))
        d_cat = dev(cat)

        def at(v):
            def run():
                ctx.config(da.Context.CFG_INFLATE_MEMBER_PARALLEL_BYTES, v)
                members(d_cat, len(cat))
            return run
        fns = {"on": at(PARALLEL_DEFAULT), "off": at(0)}
        t = alternate(fns, a.reps)
        for fn in fns.values():
            check(fn)
        at(PARALLEL_DEFAULT)()
        res["cat_64_stored_members"] = {"file_bytes": len(cat), "members": nm.value, "ms": round(t["on"][0], 3), "spread_ms": round(t["on"][1], 3),
                                        "off_ms": round(t["off"][0], 3), "off_spread_ms": round(t["off"][1], 3),
                                        "counters": ctx.inflate_members_last_parallel()}
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
