"""Sharding one input over the GPUs of a node (one process per GPU, torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" on CPU for the tests).

Two ways, DESIGN.md section 6:

* stream-exact ("P1", the default of bench.py): the ranks together produce the very bytes one
  encoder produces for the whole input.  Every rank runs links / match / parse steps on its own
  byte range (+32 KiB history, +128 KiB look-ahead) and four small exchanges place it in the global
  stream: exit tables (parse entry), token counts (+ the <= 31 743 tokens of a block that straddles
  two ranks), per-block costs (every rank then runs the same serial block plan), and the final
  OR-stitch of the packed byte ranges onto rank 0.  p1_* / encode_p1_* below.
* chunk-exact ("P2"): every rank encodes its range as one chunk, all but the last in the reference's
  sync-flush form (include/mi355_deflate.h MI355_FLUSH_SYNC), and the byte-aligned chunks are
  concatenated on rank 0.  Equal to concat_i fresh_reference_encoder(chunk_i).write_all().flush()
  (finish() for the last); matches do not cross rank boundaries.  shard_range / stitch below.
"""
import torch
import torch.distributed as dist


def shard_range(total, rank, world):
    """Contiguous, 32 KiB-aligned byte range of `rank` (the last rank takes the remainder)."""
    per = (total // world) // 32768 * 32768
    if per == 0:
        per = total // world
    lo = rank * per
    hi = total if rank == world - 1 else lo + per
    return lo, hi


def flush_mode_for(rank, world):
    return 0 if rank == world - 1 else 1  # MI355_FLUSH_FINISH / MI355_FLUSH_SYNC


def stitch(local_out, local_len, rank, world, group=None):
    """Gather the chunks onto rank 0.  local_out: uint8 tensor (device for nccl, cpu for gloo) whose
    first local_len bytes are this rank's chunk.  Returns (tensor, total_len) on rank 0, (None,
    total_len) elsewhere."""
    if world == 1:
        return local_out[:local_len], local_len
    dev = local_out.device
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([local_len], dtype=torch.int64, device=dev), group=group)
    sizes = [int(s.item()) for s in sizes]
    total = sum(sizes)
    if rank == 0:
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        buf[: sizes[0]] = local_out[: sizes[0]]
        off = sizes[0]
        reqs = []
        for r in range(1, world):
            if sizes[r]:
                reqs.append(dist.irecv(buf[off: off + sizes[r]], src=r, group=group))
            off += sizes[r]
        for q in reqs:
            q.wait()
        return buf, total
    if local_len:
        dist.send(local_out[:local_len].contiguous(), dst=0, group=group)
    return None, total


# =====================================================================================================
# Stream-exact (P1) sharding: the stitched stream equals the reference run on the WHOLE input.
# include/mi355_deflate.h ("sharded encode") describes the per-rank phases; here is what travels
# between them.  All of it is tiny next to the data: 576 x 4 bytes of exit table, 8 bytes of token
# count, at most 31743 x 4 bytes of straddling tokens and 48 bytes per block of costs per rank.
# =====================================================================================================
HISTORY = 32768          # bytes of history in front of a rank's range (the match window)
LOOKAHEAD = 128 * 1024   # bytes behind it: 258 of match look-ahead + a Stored block that begins in the range (a block of
                         # more than ~110 KB is never Stored: 31 744 tokens take less in the fixed code) -- as deflate_long.inc
BLOCK_TOKENS = 31744
ZONE = 576


SEG = 1024               # a range begins on a segment of the parse (mi355_shard_begin)


def layout_of(a, b, total, g_lo=None, g_hi=None):
    """The layout of a rank whose range is [a, b) of `total` bytes -> dict(a, b; g_lo, g_hi: the bytes it must hold; lo, hi: a, b
    in buffer coordinates).  By default one window of history in front of the range, rounded down to a whole window (the window
    geometry of the rank's buffer must be the stream's), and the look-ahead behind it."""
    if g_lo is None:
        g_lo = max(0, (a - HISTORY) // HISTORY * HISTORY)
    if g_hi is None:
        g_hi = min(total, b + LOOKAHEAD)
    return dict(a=a, b=b, g_lo=g_lo, g_hi=g_hi, lo=a - g_lo, hi=b - g_lo)


def p1_layout(total, rank, world):
    """-> dict(a, b: the rank's byte range; g_lo, g_hi: the bytes it must hold; lo, hi: a, b in buffer
    coordinates).  The ranges are shard_range's, multiples of 32 KiB, while every rank gets at least that much.  A smaller input
    is cut at multiples of 1024 bytes -- the phases take a range that begins on a segment of the parse, and nothing else --
    with the last rank taking the remainder; an input of fewer than 1024 bytes per rank cannot be cut at all: ValueError."""
    if total // world >= HISTORY:
        a, b = shard_range(total, rank, world)
    else:
        per = (total // world) // SEG * SEG
        if per == 0:
            raise ValueError("a stream-exact shard begins on a multiple of %d bytes: %d bytes are too few for %d ranks "
                             "(at least %d)" % (SEG, total, world, SEG * world))
        a = rank * per
        b = total if rank == world - 1 else a + per
    return layout_of(a, b, total)


def p1_entries(layouts, tables):
    """Entry position (global) of every rank from the exit tables: E_0 = 0, E_{r+1} = where the parse
    that enters rank r at E_r leaves it."""
    entries = []
    e = 0
    for L, X in zip(layouts, tables):
        entries.append(e)
        if e < L["b"]:
            off = e - L["a"]
            assert 0 <= off < ZONE, "entry outside the entry zone"
            e = L["b"] + X[off]
    return entries


def p1_spec_entries(layouts, specs):
    """The ranks' speculative parses, specs[r] = (held, entry, exit) in the rank's buffer coordinates: every range finds
    its entry by a run-up into its history.  If every rank's chain held and every rank was entered where the rank before it
    was left -- rank 0 at position 0 -- the entries are the true ones (induction over the ranks, as over the segments inside
    one) -> their global positions; else None: the exit tables decide (p1_entries)."""
    entries = []
    prev_exit = 0
    for L, (held, e, x) in zip(layouts, specs):
        if not held or L["g_lo"] + e != prev_exit:
            return None
        entries.append(prev_exit)
        prev_exit = L["g_lo"] + x
    return entries


def p1_token_split(counts):
    """From the token counts: for every rank (skip, tail) = how many of its first tokens belong to a block that
    began to its left, and how many tokens it needs from its right to complete its last block.
    (The form for ranges that all reach their next block boundary; p1_token_plan is the general one.)"""
    skip, tail, _, _ = p1_token_plan(counts)
    return skip, tail


def p1_token_plan(counts):
    """Blocks are every 31 744 tokens of the one global sequence; a block belongs to the rank that holds its first
    token.  -> (skip, tail, owns_final, pieces): per rank the tokens at its start that belong to a block begun
    further left (all of them, if its range does not reach the next boundary: it then owns no block), the
    tokens it needs behind its own to complete its last block, whether it owns the stream's last block, and
    where the tail comes from: [(rank, n), ...] = the first n tokens of the ranks to its right, in order."""
    world = len(counts)
    first = [0] * (world + 1)
    for r in range(world):
        first[r + 1] = first[r] + counts[r]
    T = first[world]
    final_first = T // BLOCK_TOKENS * BLOCK_TOKENS  # first token of the last block (== T: an empty last block)
    skip, tail, owns, pieces = [], [], [], []
    for r in range(world):
        lo, hi = first[r], first[r + 1]
        sk = min(counts[r], (-lo) % BLOCK_TOKENS) if r else 0
        own_lo = lo + sk                      # first token of the first block it owns, if own_lo < hi
        # (an empty last block begins "at" T: it goes to the last rank, which owns it even with no token of its own)
        of = (lo <= final_first < hi) if final_first < T else (r == world - 1)
        t = 0
        if own_lo < hi:                       # it owns at least one block
            last_first = (hi - 1) // BLOCK_TOKENS * BLOCK_TOKENS
            end = min(last_first + BLOCK_TOKENS, T)
            t = max(0, end - hi)
        pc, need, q = [], t, r + 1
        while need > 0:
            k = min(need, counts[q])
            if k:
                pc.append((q, k))
            need -= k
            q += 1
        skip.append(sk)
        tail.append(t)
        owns.append(bool(of))
        pieces.append(pc)
    return skip, tail, owns, pieces


def encode_p1_virtual(da, ctxs, data, options=None, compat=0, layouts=None):
    """All ranks in ONE process (one context per virtual rank, any devices): the same phases and the same
    exchanges as the distributed driver, with Python lists as the network.  Used by the GPU tests on a
    single-GPU box.  layouts: the ranks' layouts (layout_of) where they are not p1_layout's -- any cuts at multiples of
    1024 bytes.  Returns the stitched stream (bytes)."""
    import torch
    options = options if options is not None else da.Compression.Default
    world = len(ctxs)
    total = len(data)
    lay = list(layouts) if layouts is not None else [p1_layout(total, r, world) for r in range(world)]
    assert len(lay) == world
    bufs, shards = [], []
    try:  # (whatever happens, the contexts get their shards back: a context that holds one refuses every other encode)
        for r in range(world):
            L = lay[r]
            t = torch.frombuffer(bytearray(data[L["g_lo"]:L["g_hi"]]) + bytearray(16), dtype=torch.uint8).to(
                "cuda:%d" % ctxs[r].device)
            bufs.append(t)
            shards.append(da.Shard(ctxs[r], t.data_ptr(), L["g_hi"] - L["g_lo"], L["lo"], L["hi"], L["g_lo"], total,
                                   options, compat))
        entries = p1_spec_entries(lay, [s.spec() for s in shards])                 # exchange 0: three numbers per rank
        if entries is None:
            tables = [s.exit_table() for s in shards]                              # exchange 1 (periodic data: the exact way)
            entries = p1_entries(lay, tables)
        toks = [shards[r].emit(entries[r] - lay[r]["g_lo"]) for r in range(world)]  # (count, dptr)
        counts = [c for c, _ in toks]                                              # exchange 2
        skip, tail, owns, pieces = p1_token_plan(counts)
        costs = []
        keep = []
        for r in range(world):                                                     # exchange 3: straddling tokens
            tail_ptr = 0
            if len(pieces[r]) == 1:
                tail_ptr = toks[pieces[r][0][0]][1]
            elif pieces[r]:  # the block runs over several ranks to the right: their heads, one after the other
                t = torch.empty(tail[r], dtype=torch.int32, device=bufs[r].device)
                off = 0
                for q, k in pieces[r]:
                    ctypes_copy_d2d(t.data_ptr() + 4 * off, toks[q][1], 4 * k)
                    off += k
                keep.append(t)
                tail_ptr = t.data_ptr()
            costs.append(shards[r].blocks(skip[r], tail_ptr, tail[r], owns[r]))
        allc = [c for cs in costs for c in cs]                                     # exchange 4
        plans, total_bits = da.plan_blocks(allc, compat)
        out = torch.zeros((total_bits + 7) // 8 + 16, dtype=torch.uint8)
        b0 = 0
        for r in range(world):
            nb = len(costs[r])
            mine = plans[b0:b0 + nb]
            end_bit = plans[b0 + nb][2] if b0 + nb < len(plans) else total_bits
            b0 += nb
            if not nb:
                continue
            cap = (end_bit - mine[0][2]) // 8 + 64
            dev = torch.empty(cap, dtype=torch.uint8, device=bufs[r].device)
            fb, nbytes = shards[r].pack(mine, end_bit, dev.data_ptr(), cap)
            out[fb:fb + nbytes] |= dev[:nbytes].cpu()                             # exchange 5: OR-stitch
    finally:
        for s in shards:
            s.close()
    return bytes(out[: (total_bits + 7) // 8].numpy())


LAST_TRACE = {}  # phase times (ms) of the last encode_p1_dist on this rank, when tracing is on


def encode_p1_dist(da, ctx, d_ext, layout, total, rank, world, options=None, compat=0, group=None, comm_device=None,
                   wrapper=0, gzip_header=None, trace=None):
    """One rank of the distributed driver.  d_ext: uint8 device tensor holding bytes [g_lo, g_hi) of the
    input (+ >= 16 bytes of slack).  comm_device: where exchanged tensors live -- the GPU for the nccl
    (= RCCL) backend, "cpu" for gloo.  wrapper 1 / 2: a zlib / gzip stream (every rank sums its own range on
    its GPU, rank 0 folds the sums and frames the stitched raw stream; lib.rs:182-198, 242-267).
    Returns (tensor on rank 0 | None, stream length in bytes).  The tensor is a view of a stream image that is kept between
    calls (nothing of stream size is allocated or cleared per step): it is valid until the next call on this process --
    clone it to keep it.

    What travels, three rounds: (1) ONE all-gather of a record per rank -- "my speculative parse held,
    entered at, left at", the token count and the up to 31 743 head tokens (if the ranks' chain of entries and exits does not
    hold -- periodic data -- the 576-entry exit tables are gathered, the tokens made from the true entries and this round
    repeated), (2) ONE all-gather of a fixed-size record per rank -- block count, checksum, block costs -- after which every
    rank runs the same serial plan and knows every rank's byte range, (3) the byte ranges to rank 0, whose receives are
    posted before it packs its own blocks."""
    import ctypes
    import os
    import time

    import numpy as np
    import torch
    options = options if options is not None else da.Compression.Default
    dev = d_ext.device
    cdev = torch.device(comm_device) if comm_device is not None else dev
    L = layout
    if trace is None:
        trace = os.environ.get("MI355_P1_TRACE") == "1"
    marks = []

    def mark(name):
        if trace:
            torch.cuda.synchronize(dev)
            marks.append((name, time.perf_counter()))

    mark("start")
    sh = da.Shard(ctx, d_ext.data_ptr(), L["g_hi"] - L["g_lo"], L["lo"], L["hi"], L["g_lo"], total, options, compat,
                  torch.cuda.current_stream(dev).cuda_stream)
    mark("chains, match table, speculative parse")
    lays = [p1_layout(total, r, world) for r in range(world)]
    # round 0 + 2 in one gather: a rank's record is [token count, "my speculative parse held, entered at, left at", the head of
    # its tokens] -- the count and the head are those of the speculation's tokens, which are the tokens iff every rank's chain
    # held and every rank was entered where the rank before it was left (every rank decides the same from the same numbers).
    # (A rank may need up to 31 743 tokens from its right to complete its last block -- from the next rank, or from several
    # when their ranges are short: hence the heads.)
    HDR = 8

    def gather_counts(n_tok, tok_ptr, held, e_in, e_out):
        head_n = min(n_tok, BLOCK_TOKENS - 1)
        rec2 = torch.zeros(HDR + BLOCK_TOKENS - 1, dtype=torch.int32, device=dev)
        if head_n:
            ctypes_copy_d2d(rec2.data_ptr() + 4 * HDR, tok_ptr, head_n * 4)
        rec2[:HDR] = torch.tensor([n_tok & 0x7FFFFFFF, n_tok >> 31, int(held), e_in & 0x7FFFFFFF, e_in >> 31,
                                   e_out & 0x7FFFFFFF, e_out >> 31, 0], dtype=torch.int32)
        allr2 = torch.empty(world * rec2.numel(), dtype=torch.int32, device=cdev)
        dist.all_gather_into_tensor(allr2, rec2.to(cdev), group=group)
        allr2 = allr2.view(world, rec2.numel())
        return allr2, allr2[:, :HDR].tolist()

    held, e_in, e_out = sh.spec()
    n_tok, tok_ptr = sh.emit(e_in) if held else (0, 0)  # (returns at once: the speculation's tokens)
    all2, hdrs2 = gather_counts(n_tok, tok_ptr, held, e_in, e_out)
    entries = p1_spec_entries(lays, [(bool(h[2]), h[3] | (h[4] << 31), h[5] | (h[6] << 31)) for h in hdrs2])
    mark("x0 counts, entries and exits, straddling tokens")
    if entries is None:
        # (periodic data: the exact way) round 1: exit tables -> entry positions; the tokens from there; round 2 again
        mine = torch.tensor(sh.exit_table(), dtype=torch.int32, device=cdev)
        allv = torch.empty(world * ZONE, dtype=torch.int32, device=cdev)
        dist.all_gather_into_tensor(allv, mine, group=group)
        tables = allv.view(world, ZONE).tolist()
        entries = p1_entries(lays, tables)
        mark("x1 exit tables")
        n_tok, tok_ptr = sh.emit(entries[rank] - L["g_lo"])
        mark("emit")
        all2, hdrs2 = gather_counts(n_tok, tok_ptr, False, 0, 0)
    counts = [int(h[0]) | (int(h[1]) << 31) for h in hdrs2]
    skip, tail, owns, pieces = p1_token_plan(counts)
    tail_t = None
    if tail[rank]:
        tail_t = torch.cat([all2[q, HDR:HDR + k] for q, k in pieces[rank]]).to(dev).contiguous()
    mark("x2 counts + straddling tokens")
    # this rank's checksum (its own range only), on its GPU -- before the block phase, whose device scalars
    # the pack kernel still reads
    csum = 0
    own = L["hi"] - L["lo"]
    if wrapper == 1:
        csum = ctx.adler32_device(d_ext.data_ptr() + L["lo"], own)
    elif wrapper == 2:
        csum = ctx.crc32_device(d_ext.data_ptr() + L["lo"], own)
    nb, carr = sh.blocks_raw(skip[rank], tail_t.data_ptr() if tail_t is not None else 0, tail[rank], owns[rank])
    mark("block costs")
    # round 3: one fixed-size record per rank: [block count, checksum, costs ...] as raw bytes
    csz = ctypes.sizeof(da.BlockCost)
    per = max((lay["b"] - lay["a"]) for lay in lays) // BLOCK_TOKENS + 3  # blocks a rank can own at most
    rec = torch.zeros(16 + per * csz, dtype=torch.uint8)
    rec[:16] = torch.from_numpy(np.array([nb, csum], dtype=np.int64).view(np.uint8))
    if nb:
        if nb > per:
            raise ValueError("rank %d owns %d blocks, more than its range can hold" % (rank, nb))
        rec[16:16 + nb * csz] = torch.from_numpy(np.frombuffer(carr, dtype=np.uint8, count=nb * csz).copy())
    rec = rec.to(cdev)
    allr = torch.empty(world * rec.numel(), dtype=torch.uint8, device=cdev)
    dist.all_gather_into_tensor(allr, rec, group=group)
    allr = allr.cpu().view(world, -1).numpy()
    hdrs = allr[:, :16].copy().view(np.int64)
    nbs = [int(hdrs[r, 0]) for r in range(world)]
    sums = [int(hdrs[r, 1]) & 0xFFFFFFFF for r in range(world)]
    flat = b"".join(allr[r, 16:16 + nbs[r] * csz].tobytes() for r in range(world))
    ntot = sum(nbs)
    allc = (da.BlockCost * max(1, ntot)).from_buffer_copy(flat.ljust(csz, b"\0"))
    mark("x3 costs")
    plans, total_bits = da.plan_blocks_raw(allc, ntot, compat)
    mark("plan")
    stream_len = (total_bits + 7) // 8
    # every rank's byte range follows from the plan (mi355_shard_pack: from the 32-bit word its first block
    # starts in to the byte its last one ends in)
    starts = [sum(nbs[:r]) for r in range(world)]
    ranges = []
    for r in range(world):
        if not nbs[r]:
            ranges.append((0, 0))
            continue
        e = plans[starts[r] + nbs[r]].bit_start if starts[r] + nbs[r] < ntot else total_bits
        base = plans[starts[r]].bit_start // 32 * 32
        ranges.append((base // 8, (e - base + 7) // 8))
    b0 = starts[rank]
    end_bit = plans[b0 + nb].bit_start if b0 + nb < ntot else total_bits
    # round 4: byte ranges to rank 0, all in flight at once (every peer has its own xGMI link to rank 0), posted before
    # rank 0 packs its own blocks and received STRAIGHT INTO the stream image at their byte offsets.  Neighbours share
    # at most the 32-bit word a range starts in (mi355_shard_pack begins at a word boundary): that word -- the "head"
    # of a range -- travels on its own and is OR-ed in, everything behind it is plain data.  The image is kept
    # between steps and never cleared: only the head words are zeroed before the data of the range before them lands.
    hl = 0
    tl = {1: 4, 2: 8}.get(wrapper, 0)
    if wrapper == 1:
        hl = 2
    elif wrapper == 2:
        gzip_header = bytes(gzip_header) if gzip_header is not None else da.BLANK_GZIP_HEADER
        hl = len(gzip_header)
    reqs = []
    img = heads = None
    if rank == 0:
        img = _cached("img", cdev, hl + stream_len + 24 + tl)
        heads = _cached("heads", cdev, 4 * world)
        ops = []
        for r in range(1, world):
            f, k = ranges[r]
            if not k:
                continue
            img[hl + f:hl + f + min(4, k)].zero_()
            ops.append(dist.P2POp(dist.irecv, heads[4 * r:4 * r + min(4, k)], r, group))
            if k > 4:
                ops.append(dist.P2POp(dist.irecv, img[hl + f + 4:hl + f + k], r, group))
        reqs = dist.batch_isend_irecv(ops) if ops else []
        mark("x4 post receives")
    fb, nbytes = 0, 0
    dev_out = None
    if nb:
        cap = (end_bit - plans[b0].bit_start) // 8 + 64
        dev_out = _cached("pack", dev, cap)
        fb, nbytes = sh.pack_raw(plans, b0, end_bit, dev_out.data_ptr(), cap)
        assert (fb, nbytes) == ranges[rank]
    mark("pack")
    sh.close()
    if rank == 0:
        if nbytes:  # (rank 0's range starts the stream: nothing of a neighbour lies under it)
            img[hl + fb:hl + fb + nbytes] = dev_out[:nbytes] if cdev.type == dev.type else dev_out[:nbytes].to(cdev)
        mark("x4 own bytes")
        for q in reqs:
            q.wait()
        mark("x4 wait for the peers' bytes")
        for r in range(1, world):
            f, k = ranges[r]
            if k:
                h = min(4, k)
                img[hl + f:hl + f + h] |= heads[4 * r:4 * r + h]
        n_out = hl + stream_len
        if wrapper:
            L_ = da.load()
            acc = 1 if wrapper == 1 else 0
            for r in range(world):
                acc = L_.mi355_checksum_combine(wrapper, acc, sums[r], lays[r]["b"] - lays[r]["a"])
            if wrapper == 1:  # zlib.rs:59-62, lib.rs:192-196
                frame = torch.tensor([0x78, 0x9C], dtype=torch.uint8, device=cdev)
                trailer = torch.tensor(list(acc.to_bytes(4, "big")), dtype=torch.uint8, device=cdev)
            else:             # lib.rs:250-266
                frame = torch.tensor(list(gzip_header), dtype=torch.uint8, device=cdev)
                trailer = torch.tensor(list(acc.to_bytes(4, "little")) + list((total & 0xFFFFFFFF).to_bytes(4, "little")),
                                       dtype=torch.uint8, device=cdev)
            img[:hl] = frame
            img[n_out:n_out + trailer.numel()] = trailer
            n_out += trailer.numel()
        mark("x4 seams + framing")
        out = img[:n_out] if cdev.type == dev.type else img[:n_out].to(dev)  # (gloo dry run: the image was gathered in host memory)
        mark("x4 image to the device (gloo only)")
        if trace:
            LAST_TRACE.clear()
            LAST_TRACE.update({marks[i][0]: round(1e3 * (marks[i][1] - marks[i - 1][1]), 3) for i in range(1, len(marks))})
        return out, n_out
    if nbytes:
        src = dev_out[:nbytes] if cdev.type == dev.type else dev_out[:nbytes].to(cdev)
        ops = [dist.P2POp(dist.isend, src[:min(4, nbytes)], 0, group)]
        if nbytes > 4:
            ops.append(dist.P2POp(dist.isend, src[4:], 0, group))
        for q in dist.batch_isend_irecv(ops):
            q.wait()
    return None, stream_len + hl + tl


_CACHE = {}


def _cached(name, device, nbytes):
    """a uint8 buffer of at least nbytes on `device`, kept between steps (pinned when it is host memory)"""
    import torch
    key = (name, str(device))
    t = _CACHE.get(key)
    if t is None or t.numel() < nbytes:
        n = nbytes + nbytes // 8 + 64
        t = torch.empty(n, dtype=torch.uint8, device=device)
        if t.device.type == "cpu" and torch.cuda.is_available():
            try:
                t = t.pin_memory()
            except RuntimeError:
                pass
        _CACHE[key] = t
    return t


def ctypes_copy_d2d(dst_ptr, src_ptr, nbytes):
    """device-to-device copy of raw pointers (the token array lives in the library's workspace)"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(ctypes.c_void_p(dst_ptr), ctypes.c_void_p(src_ptr), ctypes.c_size_t(nbytes), 3)
    if rc != 0:
        raise RuntimeError("hipMemcpy D2D failed: %d" % rc)
