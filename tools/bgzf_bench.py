"""tools/bgzf_bench.py -- what the BGZF encode costs (mi355_bgzf_encode_device), on bench.py's 100 MB text at Default, device-resident.

  1. the call at block_size 65280, against mi355_deflate_encode_batch_packed_device (wrapper 2, BGZF's header, align 4, with a table)
     over the same slices, and against the single-stream gzip encode (mi355_deflate_encode_device_gzip); the three alternate in one run
  2. per stage, with the stage clocks on in a run of its own: packed encode, place, gather (mi355_bgzf_last_stages)
  3. the file's size against the single stream's: the price of blocking
  4. mi355_inflate_members_device of the file against mi355_inflate_parallel_device of the single stream

Every shape is warmed up before its timed runs; every entry returns after its stream has drained.  Per figure: best, median and
spread (max - min) over --reps runs.  Writes profiles/bgzf_bench.json unless --out says otherwise; prints ONE JSON line.
python tools/bgzf_bench.py [--reps N] [--size BYTES] [--block N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: the HIP runtime torch ships)

import datagen  # noqa: E402
import deflate_amd as da  # noqa: E402

H = bytes.fromhex("1f8b08040000000000ff0600424302000000")


def figures(ms):
    return {"best_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "runs_ms": [round(x, 4) for x in ms]}


def alternate(fns, reps):
    """every fn once to warm it, then reps rounds over all of them; host-clock ms per fn"""
    for k, fn in fns.items():
        assert fn() == 0, k
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            rc = fn()
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (k, rc)
            times[k].append(ms)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--size", type=int, default=100_000_000)
    ap.add_argument("--block", type=int, default=65280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = da.load()
    ctx = da.Context(0)
    data = datagen.text_like(a.size, 0x656E77696B38)  # (bench.py's enwik8-like text, rank 0)
    n, B = len(data), a.block
    n_slices = (n + B - 1) // B
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    o_c = da.CompressionOptions.default().to_c(2, 0, 0)
    # the BGZF call
    cap = da.bgzf_bound(n, B)
    d_file = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rows = (da.MemberInfo * (n_slices + 1))()
    file_len, n_members = C.c_size_t(0), C.c_size_t(0)
    # the packed batch over the same slices
    items = (da.BatchItem * n_slices)()
    for k in range(n_slices):
        items[k].in_, items[k].in_len = C.c_void_p(d_in.data_ptr() + k * B), min(B, n - k * B)
    hdr = (da.GzipHeader * 1)(da.GzipHeader(H, len(H)))
    p_bound = L.mi355_deflate_batch_packed_bound(items, n_slices, 2, hdr, 1, 4)
    d_arena = torch.empty(p_bound, dtype=torch.uint8, device="cuda")
    d_table = torch.empty(24 * n_slices, dtype=torch.uint8, device="cuda")
    used = C.c_size_t(0)
    # the single stream
    s_cap = L.mi355_deflate_bound_ex(n, 2, len(H), 0) + 64
    d_one = torch.empty(s_cap, dtype=torch.uint8, device="cuda")
    one_len = C.c_size_t(0)
    torch.cuda.synchronize()

    def bgzf():
        return L.mi355_bgzf_encode_device(ctx._h, C.c_void_p(d_in.data_ptr()), n, C.byref(o_c), B, C.c_void_p(d_file.data_ptr()), cap,
                                          C.byref(file_len), rows, n_slices + 1, C.byref(n_members), None)

    def packed():
        return L.mi355_deflate_encode_batch_packed_device(ctx._h, items, n_slices, C.byref(o_c), hdr, 1, C.c_void_p(d_arena.data_ptr()), p_bound, 4,
                                                          C.c_void_p(d_table.data_ptr()), C.byref(used), None)

    def single():
        return L.mi355_deflate_encode_device_gzip(ctx._h, C.c_void_p(d_in.data_ptr()), n, C.byref(o_c), da.BLANK_GZIP_HEADER,
                                                  len(da.BLANK_GZIP_HEADER), C.c_void_p(d_one.data_ptr()), s_cap, C.byref(one_len), None)

    res = {"metric": "BGZF encode, device-resident, Default (host clock around calls that return drained; %d alternating runs)" % a.reps,
           "bytes": n, "block_size": B}
    t = alternate({"bgzf": bgzf, "packed": packed, "single": single}, a.reps)
    bi = ctx.batch_info()
    res["encode"] = {k: figures(v) for k, v in t.items()}
    res["encode"]["bgzf_over_packed_median"] = round(statistics.median(t["bgzf"]) / statistics.median(t["packed"]), 4)
    res["encode"]["bgzf_minus_packed_median_ms"] = round(statistics.median(t["bgzf"]) - statistics.median(t["packed"]), 4)
    res["encode"]["bgzf_gbps_median"] = round(n / statistics.median(t["bgzf"]) / 1e6, 3)
    assert bgzf() == 0
    res["routing"] = {k: bi[k] for k in ("n_items", "n_batched", "n_single", "sub_batches")}
    res["size"] = {"file": file_len.value, "members": n_members.value, "single_stream": one_len.value, "arena_used": used.value,
                   "file_over_single": round(file_len.value / one_len.value, 5), "bound": cap}
    # the same file as Python's gzip reads it
    import gzip
    file = d_file[: file_len.value].cpu().numpy().tobytes()
    assert gzip.decompress(file) == data
    # per stage, the clocks on in a run of their own
    ctx.config(da.Context.CFG_STAGE_CLOCKS, 1)
    assert bgzf() == 0
    stages = {k: [] for k in ctx.bgzf_stages()}
    for _ in range(a.reps):
        assert bgzf() == 0
        for k, v in ctx.bgzf_stages().items():
            stages[k].append(v)
    ctx.config(da.Context.CFG_STAGE_CLOCKS, 0)
    res["stages"] = {k: figures(v) for k, v in stages.items()}
    tot = sum(statistics.median(v) for v in stages.values())
    res["stages"]["gather_share_of_call"] = round(statistics.median(stages["gather_ms"]) / tot, 4)
    res["stages"]["compressed_bytes_moved_gbps"] = round(2 * file_len.value / statistics.median(stages["gather_ms"]) / 1e6, 1)
    # decode: the members of the file against the single stream in parallel
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    got, nm, r = C.c_size_t(0), C.c_size_t(0), da.InflateReport()
    torch.cuda.synchronize()

    def members():
        return L.mi355_inflate_members_device(ctx._h, C.c_void_p(d_file.data_ptr()), file_len.value, C.c_void_p(d_out.data_ptr()), n, C.byref(got),
                                              None, 0, C.byref(nm), C.byref(r), None)

    def parallel():
        return L.mi355_inflate_parallel_device(ctx._h, C.c_void_p(d_one.data_ptr()), one_len.value, 2, C.c_void_p(d_out.data_ptr()), n, C.byref(got),
                                               C.byref(r), None)

    t = alternate({"members_of_file": members, "parallel_of_single": parallel}, a.reps)
    assert members() == 0 and got.value == n and nm.value == n_members.value and bool((d_out == d_in).all().item())
    res["decode"] = {k: figures(v) for k, v in t.items()}
    ctx.close()
    line = json.dumps(res)
    print(line)
    with open(a.out or os.path.join(ROOT, "profiles", "bgzf_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
