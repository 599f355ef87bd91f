"""tools/inflate_stream_bench.py -- what a step of many compressed connections costs through stream handles, against the one-shot batch
over the same messages.

One MI355X, device-resident data.  1, 64 and 1024 handles; each gets a message of 256 B, 4 KiB and 64 KiB of bench.py's text
(tests/datagen.py text_like) per step, sync-flushed by zlib -6 (one compressobj per connection, so a message's matches reach into the
messages before it), over 16 steps.  Timed: mi355_inflate_stream_write_batch_device, one call per step for all handles, milliseconds
per step; beside it, alternating in the same run, mi355_inflate_batch_device over the same messages compressed as independent FINISH
streams (no history, nothing carried).  The stream side pays for the history -- its copy every step, and the select in a match -- and
for re-arming the handles; the one-shot side decodes streams that compress worse because no message sees the one before it.  Medians
over steps x --reps (default 3), the best and the spread (max - min) beside them.  Connections are distinct up to 64; above that
handle h carries the bytes of connection h % 64 (the device work is the same, the host's zlib is not repeated).  Every handle's output
is compared with its message once per step, outside the timing.  Writes profiles/inflate_stream_bench.json (--out) and prints the
same JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

STEPS = 16
DISTINCT = 64


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "best_ms": round(min(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_stream_bench.json"))
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    res = {"metric": "ms per step: stream handles (write_batch_device, sync-flushed messages) against the one-shot batch (independent FINISH "
                     "streams of the same messages); medians over %d steps x %d reps, alternating" % (STEPS, a.reps),
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for size in (256, 4096, 65536):
        nd = DISTINCT
        text = datagen.text_like(nd * STEPS * size, 0x5712EA4 + size)
        msgs = [[text[(c * STEPS + s) * size:(c * STEPS + s + 1) * size] for s in range(STEPS)] for c in range(nd)]
        wire, alone = [], []
        for c in range(nd):
            z = zlib.compressobj(6, zlib.DEFLATED, -15)
            wire.append([z.compress(m) + z.flush(zlib.Z_SYNC_FLUSH) for m in msgs[c]])
            alone.append([zlib.compress(m, 6)[2:-4] for m in msgs[c]])
        d_wire = [[dev(w) for w in row] for row in wire]
        d_alone = [[dev(w) for w in row] for row in alone]
        d_msgs = [[dev(m) for m in row] for row in msgs]
        for n in (1, 64, 1024):
            outs = torch.empty(n * size, dtype=torch.uint8, device="cuda")
            hs = [ctx.inflate_stream(0) for _ in range(n)]
            harr = (C.c_void_p * n)(*[h._h for h in hs])
            s_items = [(da.BatchItem * n)() for _ in range(STEPS)]
            o_items = [(da.BatchItem * n)() for _ in range(STEPS)]
            for s in range(STEPS):
                for h in range(n):
                    c = h % nd
                    for items, src in ((s_items, d_wire), (o_items, d_alone)):
                        it = items[s][h]
                        it.in_, it.in_len = C.c_void_p(src[c][s].data_ptr()), src[c][s].numel()
                        it.out, it.out_cap = C.c_void_p(outs.data_ptr() + h * size), size

            def check(s, what):
                got = outs.view(n, size)
                for h in range(min(n, nd)):
                    assert torch.equal(got[h], d_msgs[h][s]), (what, size, n, s, h)

            t_stream, t_one = [], []
            for rep in range(a.reps + 1):  # (the first round warms)
                for h in hs:
                    h.reset()
                for s in range(STEPS):
                    for h in range(n):
                        s_items[s][h].status = o_items[s][h].status = 0
                    t0 = time.perf_counter()
                    rc = L.mi355_inflate_stream_write_batch_device(ctx._h, harr, s_items[s], n, None, None)
                    t1 = time.perf_counter()
                    assert rc == 0 and all(s_items[s][h].out_len == size for h in range(n)), (rc, size, n, s)
                    check(s, "stream")
                    outs.zero_()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    rc = L.mi355_inflate_batch_device(ctx._h, o_items[s], n, 0, None, None)
                    t3 = time.perf_counter()
                    assert rc == 0, (rc, size, n, s)
                    check(s, "one-shot")
                    outs.zero_()
                    torch.cuda.synchronize()
                    if rep:
                        t_stream.append((t1 - t0) * 1e3)
                        t_one.append((t3 - t2) * 1e3)
            for h in hs:
                h.close()
            st, one = summary(t_stream), summary(t_one)
            res["configs"]["%dx%dB" % (n, size)] = {
                "handles": n, "message_bytes": size, "wire_bytes_first_step": sum(len(wire[h % nd][0]) for h in range(n)),
                "one_shot_bytes_first_step": sum(len(alone[h % nd][0]) for h in range(n)), "stream": st, "one_shot": one,
                "stream_over_one_shot": round(st["median_ms"] / one["median_ms"], 3),
                "stream_gbps": round(n * size / st["median_ms"] / 1e6, 3)}
            del outs
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
