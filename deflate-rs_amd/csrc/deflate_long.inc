// deflate_long.inc -- inputs of any length, and streams that are never flushed, in bounded memory (SURVEY 8 row g:
// the reference takes any length in O(window) state -- it slides every 32 KiB, lz77.rs:745-756,
// input_buffer.rs:56-91, and hands bytes to the writer whenever 32 KiB are pending, compress.rs:96-124).
// Here the stream is walked as consecutive RANGES on one GPU with the phases of the sharded encode
// (deflate_shard.inc): a range is encoded from a buffer that holds 32 KiB of history before it and 128 KiB of
// look-ahead behind it; the parse enters it where the exit table of the range before says; a block belongs to
// the range that holds its first token and takes the tokens it lacks from the head of the next one, so a range
// is finished one step late, when its successor has its tokens; block types and bit offsets are planned with the
// bit position carried from range to range; the packed bytes of neighbouring ranges share their seam byte and
// are OR-ed together.  The bytes are the bytes of a single call (and of the reference): the output of the
// reference does not depend on how the input is cut into write() calls (lib.rs:408-433).
// Two contexts take the ranges in turn (the second is made on first use and belongs to the first), so that the
// tokens of a range stay where they are while the next one is worked on.  Device memory: two workspaces of
// ~20 B per byte of a range; positions are 32-bit inside a range, 64-bit between them.
constexpr uint64_t LONG_HISTORY = WINDOW_SIZE;
constexpr uint64_t LONG_LOOKAHEAD = 128 * 1024;  // 258 bytes of match look-ahead + a Stored block that begins in the range
                                                 // (a block of more than ~110 KB is never Stored: 31744 tokens in the
                                                 // fixed code take less)
constexpr uint64_t LONG_RANGE_MIN = 16ull << 20;  // >= 31744 * 258 bytes: the next range always has the tokens a block lacks
constexpr uint64_t LONG_MARGIN = 16ull << 20;     // a stream hands a range over once this much follows it (its blocks end
                                                 // well before the data known so far does)

struct LongCfg {
    uint64_t range;  // bytes per range
    uint64_t from;   // one-shot inputs of at least this many bytes go through ranges
};
// (per context: mi355_deflate_ctx_config -- defaults 512 MiB ranges, one-shot inputs beyond 1 GiB)
static LongCfg long_cfg(const mi355_deflate_ctx* c) { return LongCfg{c->long_range, c->long_from}; }
static uint64_t long_from(const mi355_deflate_ctx* c) { return c->long_from; }

// dst[i] |= src[i] for the words both hold (a seam byte is shared by two ranges), plain copy would do elsewhere
__global__ void k_or_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint64_t nwords) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nwords) {
        const uint32_t v = src[i];
        if (v) atomicOr(dst + i, v);
    }
}

struct LongEnc {
    mi355_deflate_ctx* owner = nullptr;  // the caller's context: error strings and statistics land there
    // The two contexts that take the ranges in turn.  A one-shot call works on the caller's context and one of its own; a
    // STREAM keeps a pending range -- tokens, workspace, staged input -- alive between write() calls, during which the
    // caller's (or the shared default) context may run any other encode: both of a stream's contexts are its own.
    mi355_deflate_ctx* ctx[2] = {nullptr, nullptr};
    bool own0 = false;
    mi355_deflate_opts opts;  // wrapper 0, flush 0: framing is the caller's
    bool dev_out = false;     // bytes go to a device buffer (d_out, a zeroed stream image) instead of `bytes`
    uint8_t* d_out = nullptr;
    size_t d_out_cap = 0;
    std::vector<uint8_t> bytes;  // host sink: the stream from byte `bytes_base` on (the last byte may still grow)
    uint64_t bytes_base = 0;
    uint64_t bitpos = 0;    // bits of the stream planned so far (a one-shot call starts behind its zlib / gzip header)
    uint64_t n_ranges = 0;
    uint64_t next_lo = 0;   // where the next range begins (a multiple of 32768)
    uint64_t entry = 0;     // where the parse enters it
    uint64_t tokens_before = 0;  // tokens of the stream before the pending range (or before the next one)
    mi355_shard* pend = nullptr;  // the range that waits for the head tokens of its successor
    uint64_t pend_T = 0;
    uint32_t n_blocks = 0, n_stored = 0, n_fixed = 0, n_dynamic = 0, q13_hits = 0;
    uint64_t n_tokens = 0;
    float match_ms = 0;
    int match_launches = 0;
    std::vector<mi355_block_cost> costs;
    std::vector<mi355_block_info> plans;
    uint8_t* d_tmp[2] = {nullptr, nullptr};  // packed bytes of a range
    size_t d_tmp_cap[2] = {0, 0};
    std::vector<uint8_t> h_tmp;
    // a one-shot call with a host output buffer: the ranges' bytes go straight to their place in it (the word a range starts in is
    // the only thing it shares with the range before: OR-ed where that one has written, stored elsewhere) -- a stream keeps `bytes`
    uint8_t* h_direct = nullptr;
    size_t h_cap = 0;
    uint64_t direct_end = 0;  // bytes of the buffer that hold stream data so far
};

static void long_free(LongEnc* L) {
    if (!L) return;
    if (L->pend) mi355_shard_end(L->pend);
    L->pend = nullptr;
    for (int k = 0; k < 2; k++)
        if (L->d_tmp[k]) (void)hipFree(L->d_tmp[k]);
    if (L->ctx[1]) mi355_deflate_ctx_destroy(L->ctx[1]);
    if (L->own0 && L->ctx[0]) mi355_deflate_ctx_destroy(L->ctx[0]);
    delete L;
}

static int long_new(mi355_deflate_ctx* c, const mi355_deflate_opts* o, LongEnc** out, bool for_stream) {
    LongEnc* L = new LongEnc();
    L->owner = c;
    L->ctx[0] = c;
    int rc = mi355_deflate_ctx_create(c->device, &L->ctx[1]);
    if (!rc && for_stream) {
        L->ctx[0] = nullptr;
        rc = mi355_deflate_ctx_create(c->device, &L->ctx[0]);
        L->own0 = rc == MI355_OK;
    }
    if (rc) {
        c->err = "could not create the contexts that take the ranges of a long input";
        if (L->ctx[1]) mi355_deflate_ctx_destroy(L->ctx[1]);
        delete L;
        return rc;
    }
    for (int k = 0; k < 2; k++) L->ctx[k]->sort_mode = c->sort_mode;
    L->opts = *o;
    L->opts.wrapper = 0;
    L->opts.flush = 0;
    *out = L;
    return MI355_OK;
}

// Deliver nbytes of packed output that begin at byte `first` of the deflate stream (device memory `d`, zeroed beyond).
static int long_deliver(LongEnc* L, mi355_deflate_ctx* c, const uint8_t* d, uint64_t first, size_t nbytes) {
    if (!nbytes) return MI355_OK;
    const uint64_t at = first;
    if (L->dev_out) {
        if (at + nbytes + 4 > L->d_out_cap) return MI355_E_OUT_TOO_SMALL;
        // (first is a multiple of 4: word-wise OR)
        const uint64_t nw = (nbytes + 3) / 4;
        hipLaunchKernelGGL(k_or_words, dim3((uint32_t)((nw + 255) / 256)), dim3(256), 0, c->own_stream,
                           reinterpret_cast<uint32_t*>(L->d_out + at), reinterpret_cast<const uint32_t*>(d), nw);
        HIPCHK(c, hipStreamSynchronize(c->own_stream));
        return MI355_OK;
    }
    if (L->h_direct) {
        if (at + nbytes > L->h_cap) return MI355_E_OUT_TOO_SMALL;
        uint8_t head[4] = {0, 0, 0, 0};
        const size_t h = nbytes < 4 ? nbytes : 4;
        HIPCHK(c, hipStreamSynchronize(c->own_stream));  // (the pack kernels: the threads' copies below run on streams of their own)
        HIPCHK(c, hipMemcpy(head, d, h, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h; i++) {
            const uint64_t p = at + i;
            L->h_direct[p] = p < L->direct_end ? (uint8_t)(L->h_direct[p] | head[i]) : head[i];
        }
        if (nbytes > 4) {
            // (pageable memory: through the context's host threads, deflate_bounce.inc)
            if (bounce_out(c, L->h_direct + at + 4, d + 4, nbytes - 4)) {
                if (!bounce_close(c, false)) {
                    c->err = "host threads: a copy of the output failed";
                    return MI355_E_HIP;
                }
            } else {
                HIPCHK(c, hipMemcpy(L->h_direct + at + 4, d + 4, nbytes - 4, hipMemcpyDeviceToHost));
            }
        }
        if (at + nbytes > L->direct_end) L->direct_end = at + nbytes;
        return MI355_OK;
    }
    // (the word the range starts in is all it shares with the bytes before it: those few bytes are OR-ed in, the rest is this
    // range's alone and goes straight into the vector -- through the host threads when it is large)
    uint8_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t h = nbytes < 8 ? nbytes : 8;
    HIPCHK(c, hipStreamSynchronize(c->own_stream));
    HIPCHK(c, hipMemcpy(head, d, h, hipMemcpyDeviceToHost));
    // the packed bytes begin at a word boundary: up to three bytes in front of the range's first bit, which have been
    // handed out already when a stream drains as it goes -- this range has no bit in them
    size_t lead = 0;
    if (at < L->bytes_base) {
        lead = (size_t)(L->bytes_base - at);
        if (lead > 3 || lead > nbytes) return MI355_E_ARG;
        for (size_t i = 0; i < lead; i++)
            if (head[i]) return MI355_E_ARG;
    }
    const uint64_t off = at + lead - L->bytes_base;
    if (off + (nbytes - lead) > L->bytes.size()) L->bytes.resize((size_t)(off + nbytes - lead), 0);
    for (size_t i = lead; i < h; i++) L->bytes[(size_t)(off + i - lead)] |= head[i];
    if (nbytes > h) {
        uint8_t* dst = L->bytes.data() + (size_t)(off + h - lead);
        if (bounce_out(c, dst, d + h, nbytes - h)) {
            if (!bounce_close(c, false)) {
                c->err = "host threads: a copy of the output failed";
                return MI355_E_HIP;
            }
        } else {
            HIPCHK(c, hipMemcpy(dst, d + h, nbytes - h, hipMemcpyDeviceToHost));
        }
    }
    return MI355_OK;
}

// Blocks, plan, pack and delivery of range `s` (T own tokens, the first of them token number `first` of the stream);
// `tail_ptr` / `tail_avail`: head tokens of the range behind it; `stream_T`: tokens of the whole stream if it ends
// with the range behind (or with this one), else 0; `end_mode`: 0 = the stream goes on, 1 = finish, 2 = sync flush.
static int long_finish_range(LongEnc* L, mi355_shard* s, uint64_t T, uint64_t first, const void* tail_ptr, uint64_t tail_avail,
                             uint64_t stream_T, int end_mode, bool is_last) {
    mi355_deflate_ctx* c = s->c;
    const uint64_t B = MAX_BUFFER_LENGTH;
    const uint64_t skip = first ? std::min<uint64_t>(T, (B - first % B) % B) : 0;
    const uint64_t own_lo = first + skip, hi = first + T;
    uint64_t tail = 0;
    bool owns_final = false;
    if (end_mode) {
        // the last block begins at the last multiple of 31744 tokens; when that is the end of the stream it is empty
        // (compress.rs:247-261 writes a block whenever the parser reports Finished) and belongs to the last range
        const uint64_t final_first = stream_T / B * B;
        owns_final = final_first < stream_T ? (first <= final_first && final_first < hi) : is_last;
    }
    if (own_lo < hi) {
        const uint64_t last_first = (hi - 1) / B * B;
        uint64_t end = last_first + B;
        if (end_mode && end > stream_T) end = stream_T;
        tail = end > hi ? end - hi : 0;
    }
    if (tail > tail_avail) return MI355_E_ARG;  // (ranges are long enough: LONG_RANGE_MIN)
    // an empty last block "at" stream_T belongs to the last range even when it has no token of its own left
    uint64_t nb = 0;
    L->costs.resize((size_t)((T + tail) / B + 2));
    int rc = mi355_shard_blocks_ex(s, skip, tail_ptr, tail, owns_final ? 1 : 0, &nb, L->costs.data(), L->costs.size());
    if (rc) return rc;
    if (nb == 0) return MI355_OK;
    L->plans.resize((size_t)nb);
    for (uint64_t b = 0; b < nb; b++) {
        BlockPlan p;
        const bool last = owns_final && b + 1 == nb;
        plan_block(L->costs[b].dyn_bits, L->costs[b].dyn_est, L->costs[b].static_est, L->costs[b].fixed_bits, L->costs[b].in_bytes,
                   last && end_mode == 1, L->bitpos, &p);
        if (p.btype == BT_STORED && L->costs[b].q13 == 2 && (L->opts.compat & MI355_COMPAT_Q13)) return MI355_E_REF_PANIC;
        L->plans[b].btype = p.btype;
        L->plans[b].bfinal = p.bfinal;
        L->plans[b].n_tokens = 0;
        L->plans[b].reserved = 0;
        L->plans[b].in_bytes = L->costs[b].in_bytes;
        L->plans[b].bit_start = p.bit_start;
        L->bitpos += p.bit_len;
        L->n_blocks++;
        L->n_stored += p.btype == BT_STORED;
        L->n_fixed += p.btype == BT_FIXED;
        L->n_dynamic += p.btype == BT_DYNAMIC;
        L->q13_hits += L->costs[b].q13 != 0;
    }
    const int k = (c == L->ctx[1]) ? 1 : 0;
    const uint64_t base_bit = L->plans[0].bit_start / 32 * 32;
    const size_t need = (size_t)((L->bitpos - base_bit + 7) / 8) + 64;
    if (need > L->d_tmp_cap[k]) {
        if (L->d_tmp[k]) (void)hipFree(L->d_tmp[k]);
        L->d_tmp[k] = nullptr;
        L->d_tmp_cap[k] = 0;
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&L->d_tmp[k]), need + need / 8));
        L->d_tmp_cap[k] = need + need / 8;
    }
    uint64_t fb = 0;
    size_t nbytes = 0;
    rc = mi355_shard_pack(s, L->plans.data(), L->bitpos, L->d_tmp[k], L->d_tmp_cap[k], &fb, &nbytes);
    if (rc) return rc;
    return long_deliver(L, c, L->d_tmp[k], fb, nbytes);
}

// One more range: d_ext = the bytes [g_lo, g_lo + n_ext) of the stream on the device of the contexts, the range itself
// is [g_lo + lo, g_lo + hi); `end_mode` != 0: the stream ends with this range (1 = finish, 2 = sync flush) at
// g_lo + n_ext = n_stream, else n_stream = the end of the data known so far.
// (skew / holes: the range begins at a sync-flush point of a stream -- the positions the write calls around the flush filed
// differently, in buffer coordinates; such a range begins anywhere, all others at a multiple of 32768)
static int long_range(LongEnc* L, const uint8_t* d_ext, uint64_t n_ext, uint64_t lo, uint64_t hi, uint64_t g_lo, uint64_t n_stream,
                      int end_mode, const ShardQuirks* quirks = nullptr) {
    const int k = (int)(L->n_ranges & 1);
    mi355_deflate_ctx* c = L->ctx[k];
    mi355_shard* s = nullptr;
    int rc = shard_begin_at(c, d_ext, (size_t)n_ext, (size_t)lo, (size_t)hi, g_lo, n_stream, &L->opts, nullptr, &s, quirks);
    if (rc) {
        if (c != L->owner) L->owner->err = c->err;
        return rc;
    }
    L->n_ranges++;
    L->match_ms += c->info.match_ms;
    L->match_launches += c->info.match_launches;
    auto fail = [&](int r) {
        if (c != L->owner) L->owner->err = c->err;
        mi355_shard_end(s);
        return r;
    };
    const uint64_t a = g_lo + lo, b = g_lo + hi;
    const uint64_t entry = L->entry;
    uint64_t next_entry = entry;
    // the range was parsed by speculation in mi355_shard_begin: if that entered it where the range before was left, its tokens
    // are there and its exit is the next entry; else the exit table says where this entry leads (the exact way)
    int held = 0;
    uint64_t s_in = 0, s_out = 0;
    rc = mi355_shard_spec(s, &held, &s_in, &s_out);
    if (rc) return fail(rc);
    if (held && g_lo + s_in == entry) {
        next_entry = g_lo + s_out;
    } else if (entry < b) {
        uint32_t X[ZONE];
        rc = mi355_shard_exit_table(s, X);
        if (rc) return fail(rc);
        if (entry < a || entry - a >= ZONE) return fail(MI355_E_ARG);
        next_entry = b + X[entry - a];
    }
    uint64_t T = 0;
    const void* dtok = nullptr;
    rc = mi355_shard_emit(s, entry - g_lo, &T, &dtok);
    if (rc) return fail(rc);
    L->n_tokens += T;
    // the range before can be finished now: its last block is completed from this range's first tokens
    if (L->pend) {
        const uint64_t first = L->tokens_before;
        const uint64_t stream_T = end_mode ? first + L->pend_T + T : 0;
        rc = long_finish_range(L, L->pend, L->pend_T, first, dtok, T, stream_T, end_mode, false);
        mi355_shard_end(L->pend);
        L->pend = nullptr;
        if (rc) return fail(rc);
        L->tokens_before += L->pend_T;
    }
    L->entry = next_entry;
    L->next_lo = b;
    if (end_mode) {
        const uint64_t first = L->tokens_before;
        rc = long_finish_range(L, s, T, first, nullptr, 0, first + T, end_mode, true);
        mi355_shard_end(s);
        if (rc) return rc;
        L->tokens_before += T;
        if (end_mode == 2) {  // compress.rs:256-261: an empty stored block, not final -- 3 header bits, pad, 00 00 FF FF
            L->bitpos = (L->bitpos + 3 + 7) / 8 * 8;
            if (L->dev_out) {  // (the image is zeroed: header bits, padding and LEN are there)
                const uint8_t nlen[2] = {0xFF, 0xFF};
                if (L->bitpos / 8 + 4 > L->d_out_cap) return MI355_E_OUT_TOO_SMALL;
                HIPCHK(L->owner, hipMemcpy(L->d_out + L->bitpos / 8 + 2, nlen, 2, hipMemcpyHostToDevice));
            } else if (L->h_direct) {  // (what the stream has not reached yet is not zero in the caller's buffer)
                const uint64_t off = L->bitpos / 8;
                if (off + 4 > L->h_cap) return MI355_E_OUT_TOO_SMALL;
                for (uint64_t p = L->direct_end; p < off + 2; p++) L->h_direct[p] = 0;
                L->h_direct[off + 2] = 0xFF;
                L->h_direct[off + 3] = 0xFF;
                if (off + 4 > L->direct_end) L->direct_end = off + 4;
            } else {
                const uint64_t off = L->bitpos / 8 - L->bytes_base;
                if (L->bytes.size() < off + 4) L->bytes.resize((size_t)off + 4, 0);
                L->bytes[(size_t)off + 2] = 0xFF;
                L->bytes[(size_t)off + 3] = 0xFF;
            }
            L->bitpos += 32;
        }
        return MI355_OK;
    }
    L->pend = s;
    L->pend_T = T;
    return MI355_OK;
}

// ---- a whole input that is resident on the device or in host memory --------------------------------------------
// d_in != nullptr: device input; else h_in.  Output: device buffer d_out (zeroed here) or host buffer h_out.
static int encode_long(mi355_deflate_ctx* c, const uint8_t* d_in, const uint8_t* h_in, uint64_t n, const mi355_deflate_opts* o,
                       uint8_t* d_out, uint8_t* h_out, size_t out_cap, size_t* out_len, const uint8_t* gz_hdr, size_t gz_len) {
    if (o->flush > MI355_FLUSH_SYNC) return MI355_E_ARG;
    const bool sync = o->flush == MI355_FLUSH_SYNC;  // (header, every block non-final, the sync marker, no trailer: run_encode)
    const bool zlib = o->wrapper == 1, gzip = o->wrapper == 2;
    if (o->wrapper > 2 || (gzip && (!gz_hdr || gz_len == 0 || gz_len > 0xFFFF))) return MI355_E_ARG;
    if (!gzip) gz_len = 0;
    const size_t need_out = mi355_deflate_bound_ex(n, o->wrapper, gz_len, 0);
    if (out_cap < need_out) {
        *out_len = need_out;
        c->err = "output buffer smaller than mi355_deflate_bound_ex(in_len, wrapper, hdr_len, 0)";
        return MI355_E_OUT_TOO_SMALL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    LongEnc* L = nullptr;
    int rc = long_new(c, o, &L, false);
    if (rc) return rc;
    const size_t hdr = zlib ? 2 : gz_len;
    L->bitpos = 8 * (uint64_t)hdr;  // (block phases only see the bit position modulo 8)
    L->dev_out = d_out != nullptr;
    L->d_out = d_out;
    L->d_out_cap = out_cap;
    if (!d_out) {
        L->h_direct = h_out;
        L->h_cap = out_cap;
    }
    if (d_out) HIPCHK(c, hipMemsetAsync(d_out, 0, need_out, c->own_stream));
    const LongCfg cfg = long_cfg(c);
    uint32_t sum = zlib ? 1u : 0u;
    uint64_t a = 0;
    Arrival arrival;
    while (rc == MI355_OK) {
        uint64_t b = a + cfg.range;
        if (n - a < cfg.range + LONG_RANGE_MIN) b = n;  // the last range takes a short remainder with it
        const bool last = b == n;
        const uint64_t g_lo = a >= LONG_HISTORY ? a - LONG_HISTORY : 0, g_hi = last ? n : std::min<uint64_t>(n, b + LONG_LOOKAHEAD);
        const int k = (int)(L->n_ranges & 1);
        mi355_deflate_ctx* ck = L->ctx[k];
        const uint8_t* d_ext = nullptr;
        if (d_in) {
            d_ext = d_in + g_lo;
        } else {
            rc = ensure_buf(ck, &ck->d_in, &ck->d_in_cap, (size_t)(g_hi - g_lo) + 64);
            if (rc) break;
            // the range goes over the bus in pieces and its tables start on the first one (as a rank of the multi-GPU call does:
            // deflate_multi.inc) -- pageable memory through the context's host threads (deflate_bounce.inc)
            ck->next_arrival = nullptr;
            if (g_hi - g_lo >= HOST_PIECEWISE_FROM) {
                rc = arrive_in_pieces(ck, ck->d_in, h_in + g_lo, g_hi - g_lo, arrival, 0, HOST_PIECES, true);
                if (rc) break;
                ck->next_arrival = &arrival;
            } else if (hipMemcpy(ck->d_in, h_in + g_lo, (size_t)(g_hi - g_lo), hipMemcpyHostToDevice) != hipSuccess) {
                rc = fail_hip(c, "hipMemcpy(range)", hipGetLastError());
                break;
            }
            d_ext = ck->d_in;
        }
        rc = long_range(L, d_ext, g_hi - g_lo, a - g_lo, b - g_lo, g_lo, n, last ? (sync ? 2 : 1) : 0);
        if (!d_in) {  // (the threads are done with the caller's range, or told to drop the rest)
            ck->next_arrival = nullptr;
            if (!bounce_close(ck, rc != MI355_OK) && rc == MI355_OK) {
                ck->err = "host threads: a copy of the input failed";
                rc = MI355_E_HIP;
            }
            if (ck->copy_stream) (void)hipStreamSynchronize(ck->copy_stream);
            if (rc && ck != c) c->err = ck->err;
        }
        if (rc) break;
        if (zlib || gzip) {  // the checksum of the range's own bytes, folded into the stream's (behind the tables: they have waited for
                             // the range's last piece)
            uint32_t part = 0;
            rc = gzip ? mi355_crc32_device(ck, d_ext + (a - g_lo), (size_t)(b - a), &part, nullptr)
                      : mi355_adler32_device(ck, d_ext + (a - g_lo), (size_t)(b - a), &part, nullptr);
            if (rc) break;
            sum = gzip ? crc_combine(sum, part, b - a) : adler_combine(sum, part, b - a);
        }
        a = b;
        if (last) break;
    }
    if (rc == MI355_OK) {
        const size_t upto = (size_t)((L->bitpos + 7) / 8);  // header and deflate stream
        uint8_t head[4] = {0x78, 0x9C, 0, 0};
        uint8_t trail[8];
        size_t ntrail = 0;
        if (sync) {
        } else if (zlib) {  // lib.rs:192-196: Adler-32 big endian
            trail[0] = (uint8_t)(sum >> 24);
            trail[1] = (uint8_t)(sum >> 16);
            trail[2] = (uint8_t)(sum >> 8);
            trail[3] = (uint8_t)sum;
            ntrail = 4;
        } else if (gzip) {  // lib.rs:258-266: CRC-32 and the length mod 2^32, little endian
            for (int i = 0; i < 4; i++) trail[i] = (uint8_t)(sum >> (8 * i));
            for (int i = 0; i < 4; i++) trail[4 + i] = (uint8_t)((uint32_t)n >> (8 * i));
            ntrail = 8;
        }
        const size_t total = upto + ntrail;
        if (total > out_cap) {
            rc = MI355_E_OUT_TOO_SMALL;
        } else if (d_out) {
            // (the header's bytes of the image are zero: the first block was OR-ed in behind them)
            if (hdr) HIPCHK(c, hipMemcpy(d_out, zlib ? head : gz_hdr, hdr, hipMemcpyHostToDevice));
            if (ntrail) HIPCHK(c, hipMemcpy(d_out + upto, trail, ntrail, hipMemcpyHostToDevice));
        } else {
            // (the ranges' bytes are in place; what the stream did not reach -- a stream that ends in the sync marker's zero bytes,
            // an empty input -- is cleared)
            for (uint64_t p = L->direct_end; p < upto; p++) h_out[p] = 0;
            if (hdr) memcpy(h_out, zlib ? head : gz_hdr, hdr);
            if (ntrail) memcpy(h_out + upto, trail, ntrail);
        }
        if (rc == MI355_OK) {
            *out_len = total;
            mi355_deflate_info& info = c->info;
            memset(&info, 0, sizeof info);
            c->pend_passes = 0;
            info.in_len = n;
            info.out_len = total;
            info.n_tokens = L->n_tokens;
            info.n_blocks = L->n_blocks;
            info.n_stored = L->n_stored;
            info.n_fixed = L->n_fixed;
            info.n_dynamic = L->n_dynamic;
            info.q13_hits = L->q13_hits;
            info.passes = (uint32_t)L->n_ranges;
            info.match_ms = L->match_ms;
            info.match_launches = L->match_launches;
            info.stage_ms[MI355_STAGE_MATCH] = L->match_ms;
            c->last_plan = nullptr;
            c->last_nb = 0;
        }
    }
    long_free(L);
    return rc;
}

// ---- the streaming handle: a stream that has not been flushed yet hands its ranges over as they fill up ---------
// (mi355_deflate_stream_write calls stream_pump after it has taken the bytes; flush() / finish() of such a stream end
// it with stream_long_end.)  What the handle holds: the range being gathered, the margin behind it, one window of
// history, and the bytes not yet taken.
// A stream that has been flushed does the same with what is written after its last flush point F (= s->emitted): the first
// range begins AT F -- the parse starts there afresh, the blocks count from there, the stream is byte aligned -- with the
// window in front of it and the hash quirks of the write calls around the flush (stages.h HashOverride); the next flush() /
// finish() ends the last range.  (F inside the first three windows: the start of a stream has rules of its own -- Q1, hash
// re-warm at flush points -- and such a chunk is encoded in one call, which takes less than 4 GiB - 64 KiB.)
static bool stream_long_eligible(const mi355_deflate_stream* s) {
    if (s->L != nullptr) return true;
    if (s->flush_points.empty() && s->emitted == 0 && s->base == 0 && !s->after_flush) return true;
    return !s->flush_points.empty();
}

// hand the deflate bytes that are complete over to the stream's output
static void stream_long_drain(mi355_deflate_stream* s, bool all) {
    LongEnc* L = s->L;
    const uint64_t done = all ? (L->bitpos + 7) / 8 : L->bitpos / 8;  // (the byte the next block starts in may still grow)
    if (done <= L->bytes_base) return;
    const size_t k = (size_t)(done - L->bytes_base);
    if (L->bytes.size() < k) L->bytes.resize(k, 0);
    s->output.insert(s->output.end(), L->bytes.begin(), L->bytes.begin() + k);
    L->bytes.erase(L->bytes.begin(), L->bytes.begin() + k);
    L->bytes_base = done;
}

// one range [a, b) of the stream (end_mode != 0: the rest of it, b = total) from the handle's buffer
static int stream_long_range(mi355_deflate_stream* s, uint64_t a, uint64_t b, int end_mode) {
    mi355_deflate_ctx* c = s->ctx;
    if (!s->L) {
        int rc = long_new(c, &s->opts, &s->L, true);
        if (rc) return rc;
        s->L->entry = s->L->next_lo = a;  // (0, or the flush point the ranges begin at)
    }
    LongEnc* L = s->L;
    HIPCHK(c, hipSetDevice(c->device));
    // (a range that begins inside the first three windows -- at an early flush point -- holds the stream from its start: a hash
    // re-warmed at the stream's start is a candidate up to position 65537; the handle keeps the stream's start that long too)
    const uint64_t g_lo = a >= 3ull * WINDOW_SIZE ? (a - LONG_HISTORY) / WINDOW_SIZE * WINDOW_SIZE : 0;
    const uint64_t g_hi = end_mode ? s->total : std::min<uint64_t>(s->total, b + LONG_LOOKAHEAD);
    if (g_lo < s->base) return MI355_E_STATE;
    mi355_deflate_ctx* ck = L->ctx[L->n_ranges & 1];
    int rc = ensure_buf(ck, &ck->d_in, &ck->d_in_cap, (size_t)(g_hi - g_lo) + 64);
    if (rc) return rc;
    if (g_hi > g_lo)
        HIPCHK(c, hipMemcpy(ck->d_in, s->win.data() + (g_lo - s->base), (size_t)(g_hi - g_lo), hipMemcpyHostToDevice));
    if (s->opts.wrapper != 0 && b > a) {
        uint32_t part = 0;
        rc = s->opts.wrapper == 2 ? mi355_crc32_device(ck, ck->d_in + (a - g_lo), (size_t)(b - a), &part, nullptr)
                                  : mi355_adler32_device(ck, ck->d_in + (a - g_lo), (size_t)(b - a), &part, nullptr);
        if (rc) return rc;
        s->adler = s->opts.wrapper == 2 ? crc_combine(s->adler, part, b - a) : adler_combine(s->adler, part, b - a);
        s->summed += b - a;
    }
    if (g_hi == g_lo) {  // (an empty stream never gets here: it takes the plain path)
        return MI355_E_STATE;
    }
    std::vector<uint32_t> skew, holes;
    ShardQuirks quirks;
    const bool at_flush = L->n_ranges == 0 && a > 0;  // the range begins at a flush point
    if (at_flush) {
        for (uint64_t f : s->skew)
            if (f >= g_lo && f < g_hi) skew.push_back((uint32_t)(f - g_lo));
        for (uint64_t f : s->holes)
            if (f >= g_lo && f < g_hi) holes.push_back((uint32_t)(f - g_lo));
        quirks.skew = &skew;
        quirks.holes = &holes;
        if (g_lo == 0) {  // ... inside the first windows of the stream: what its flush calls passed to the single pass
            quirks.rewarm = &s->rewarm;
            quirks.q1_on = s->q1_on;
            quirks.q1_pos = s->q1_pos;
        }
    }
    rc = long_range(L, ck->d_in, g_hi - g_lo, a - g_lo, b - g_lo, g_lo, s->total, end_mode, at_flush ? &quirks : nullptr);
    if (rc) return rc;
    stream_long_drain(s, end_mode != 0);
    return MI355_OK;
}

static int stream_pump(mi355_deflate_stream* s) {
    const LongCfg cfg = long_cfg(s->ctx);
    for (;;) {
        const uint64_t a = s->L ? s->L->next_lo : s->emitted;  // (a stream that was never flushed: 0)
        if (s->total - a < cfg.range + LONG_MARGIN + LONG_LOOKAHEAD) return MI355_OK;
        const uint64_t b = (a + cfg.range) / WINDOW_SIZE * WINDOW_SIZE;  // (a range that begins at a flush point ends at a multiple too)
        int rc = stream_long_range(s, a, b, 0);
        if (rc) return rc;
        // let go of what no later range can see: the next one starts at b with one window of history
        const uint64_t want = b - LONG_HISTORY;
        if (want > s->base) {
            s->win.erase(s->win.begin(), s->win.begin() + (size_t)(want - s->base));
            s->base = want;
        }
    }
}

// flush() (mode 2) or finish() (mode 1) of a stream that has handed ranges over: the rest is its last range
static int stream_long_end(mi355_deflate_stream* s, int mode) {
    LongEnc* L = s->L;
    const uint64_t a = L->next_lo;
    int rc = stream_long_range(s, a, s->total, mode);
    if (rc) return rc;
    long_free(L);
    s->L = nullptr;
    s->emitted = s->total;
    return MI355_OK;
}

extern "C" {

// Tuning of a context (include/mi355_deflate.h).
int mi355_deflate_ctx_config(mi355_deflate_ctx* c, int key, uint64_t value) {
    // (like the argument errors of the calls it tunes: decided before a context or the device is touched)
    if (key == MI355_CFG_INFLATE_INDEX_SPAN_BYTES && (value < 256 || value > (1ull << 30))) return MI355_E_ARG;
    if (key == MI355_CFG_INFLATE_MEMBER_SPAN_BYTES && (value < 16 || value > (1ull << 30))) return MI355_E_ARG;
    if (key == MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES && value && (value < 1024 || value > (1ull << 30))) return MI355_E_ARG;
    if (key == MI355_CFG_INFLATE_SEEK_CUT_BYTES && value && (value < 64 || value > (1ull << 30))) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    switch (key) {
    case MI355_CFG_RANGE_BYTES: {
        uint64_t r = (value < LONG_RANGE_MIN ? LONG_RANGE_MIN : value) / WINDOW_SIZE * WINDOW_SIZE;
        if (r > 0xC0000000ull) r = 0xC0000000ull;  // 3 GiB: a range and its halo stay below 4 GiB - 64 KiB
        c->long_range = r;
        return MI355_OK;
    }
    case MI355_CFG_LONG_FROM:
        if (value == 0 || value > 0xFFFF0000ull) return MI355_E_ARG;  // (a single pass takes less than 4 GiB - 64 KiB)
        c->long_from = value;
        return MI355_OK;
    case MI355_CFG_MULTI_STITCH:
        if (value > 1) return MI355_E_ARG;
        c->multi_stitch = (int)value;
        return MI355_OK;
    case MI355_CFG_STEPS_IN_EMIT:
        if (value > 1) return MI355_E_ARG;
        c->steps_in_emit = (int)value;
        return MI355_OK;
    case MI355_CFG_HOST_BOUNCE:
        if (value > 1) return MI355_E_ARG;
        c->host_bounce = (int)value;
        return MI355_OK;
    case MI355_CFG_HOST_THREADS:
        if (value < 1 || value > (uint64_t)BOUNCE_THREADS_MAX) return MI355_E_ARG;
        if (c->bounce) return MI355_E_STATE;
        c->host_threads = (int)value;
        return MI355_OK;
    case MI355_CFG_HOST_STREAMING:
        if (value > 2) return MI355_E_ARG;
        c->host_streaming = (int)value;
        return MI355_OK;
    case MI355_CFG_STAGE_CLOCKS:
        if (value > 2) return MI355_E_ARG;
        c->stage_clocks = (int)value;
        return MI355_OK;
    case MI355_CFG_BATCH_BYTES:
        if (value < (1ull << 20) || value > (1ull << 30)) return MI355_E_ARG;
        c->batch_bytes = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_GROUP_BYTES:
        if (value < (64ull << 10)) return MI355_E_ARG;
        c->inflate_group_bytes = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_INDEX_SPAN_BYTES:
        c->index_span = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_MEMBER_SPAN_BYTES:
        c->member_span = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_MEMBER_PARALLEL_BYTES:
        c->member_parallel = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_SEEK_CUT_BYTES:
        c->seek_cut_bytes = value;
        return MI355_OK;
    case MI355_CFG_INFLATE_SEEK_CUT_WALKER:
        if (value > 1) return MI355_E_ARG;
        c->seek_cut_walker = value;
        return MI355_OK;
    case MI355_CFG_SORT_RANKS:
        if (value > 1) return MI355_E_ARG;
        if (value == 1 && !c->lds_order_ok) return MI355_E_UNSUPPORTED;  // the device failed the self-test
        c->sort_mode = (int)value;
        return MI355_OK;
    default: return MI355_E_ARG;
    }
}

// what a key of the decode side is set to (the keys 11 to 16; any other: MI355_E_ARG)
int mi355_deflate_ctx_config_get(mi355_deflate_ctx* c, int key, uint64_t* value) {
    if (!value || key < MI355_CFG_INFLATE_GROUP_BYTES || key > MI355_CFG_INFLATE_SEEK_CUT_WALKER) return MI355_E_ARG;
    DefaultGuard dg_;
    c = use_ctx(c, dg_);
    if (!c) return MI355_E_HIP;
    const uint64_t v[6] = {c->inflate_group_bytes, c->index_span, c->member_span, c->member_parallel, c->seek_cut_bytes, c->seek_cut_walker};
    *value = v[key - MI355_CFG_INFLATE_GROUP_BYTES];
    return MI355_OK;
}

// what a stream handle holds in host memory: gathered input, window, bytes not yet taken
uint64_t mi355_deflate_stream_held_bytes(mi355_deflate_stream* s) {
    if (!s) return 0;
    return (uint64_t)s->win.size() + (uint64_t)(s->output.size() - s->taken) + (s->L ? (uint64_t)s->L->bytes.size() : 0);
}

#ifdef MI355_DEBUG_HOOKS
// test build only (libmi355deflate_dbg.so): make k_sort<1> of this context hand out wrong ranks, as a device would whose
// LDS did not serve same-address lanes in lane order -- the walk's order check must catch it
int mi355_debug_break_sort(mi355_deflate_ctx* c, int on) {
    if (!c) return MI355_E_ARG;
    c->sort_break = on ? 1 : 0;
    return MI355_OK;
}
int mi355_debug_sort_ranks(mi355_deflate_ctx* c) { return c ? c->sort_mode : -1; }
// test build only: the sort's tables of the context's last single-pass call, as they lie in its workspace -- `ne` epochs from
// e0 on, 32 768 entries of S (2 x position) and BSTRIDE entries of B each.  (Allocations of their own: nothing behind the walk
// writes them.)
int mi355_debug_sort_tables(mi355_deflate_ctx* c, uint32_t e0, uint32_t ne, uint16_t* S_out, uint16_t* B_out) {
    if (!c || (ne && (!S_out || !B_out))) return MI355_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->own_stream) != hipSuccess) return MI355_E_HIP;
    if (!c->dbg_sorted || (uint64_t)e0 + ne > c->dbg_epochs) {
        c->err = "the workspace holds fewer sorted epochs than asked for";
        return MI355_E_ARG;
    }
    if (ne == 0) return MI355_OK;
    if (hipMemcpy(S_out, c->dbg_sorted + (size_t)e0 * WINDOW_SIZE, (size_t)ne * WINDOW_SIZE * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(B_out, c->dbg_buckets + (size_t)e0 * BSTRIDE, (size_t)ne * BSTRIDE * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess)
        return MI355_E_HIP;
    return MI355_OK;
}
// test build only: 1 = k_sort marks every epoch with 1024 or more positions for the permuted pair table (k_match3_swz) whatever
// its samples say -- a state that data could produce --, 2 = it marks none, 0 = by the samples
int mi355_debug_force_swz(mi355_deflate_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return MI355_E_ARG;
    c->force_swz = mode;
    return MI355_OK;
}
#endif

}  // extern "C"
